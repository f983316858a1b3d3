"""Static instruction census of one solver instantiation, phase by phase (no GPU needed): the translation unit is compiled to assembly with the
phase clocks of `make TRACE=1` in, and the instructions between successive clock reads are counted by class.  A lone solver wave issues one
instruction per ~4.4 clocks whatever its class, so these counts ARE the cost model of the iteration.
    python tools/asm_census.py NOBS NMAX DEG NFIX [extra hipcc flags]     e.g.  python tools/asm_census.py 1 12 6 12 -DCRX_STATIC_LDS=0
Loop bodies are counted once (a rolled Riccati stage loop = one `ric k:` group, executed N times per factorisation; an unrolled sweep prints every stage).
Two columns price what the issue slots and the LDS waits are spent on besides arithmetic: `spill` = v_writelane / v_readlane on the VGPRs that carry
spilled SGPRs (the registers some v_writelane_b32 of the build writes), `xwait` = s_waitcnt on the LDS counter that follow the last LDS load in front
of them by <= 3 instructions (a round trip with nothing to hide it: a lone wave has no other wave to run meanwhile)."""
import os, re, subprocess, sys, tempfile
from collections import Counter
ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recipe
tpl = ",".join(sys.argv[1:5]); extra = sys.argv[5:]
# csrc/crx_kernels_one.hip with the flags of the unit that ships the instantiation, as the Makefile's recipe states them
unit = "crx_kernels_one_obs.o" if sys.argv[1] != "0" else "crx_kernels_one_plan.o"
def build(flags):
    out = tempfile.mktemp(suffix=".s")
    cmd = recipe.command(unit, ["-DCRX_PROBE_ONE=" + tpl] + flags + extra)
    subprocess.run(cmd[:-1] + ["--cuda-device-only", "-S", cmd[-1], "-o", out], check=True, stderr=subprocess.DEVNULL)
    t = open(out).read().split("\n"); os.unlink(out)
    return t
def isins(x):
    s = x.strip()
    return x.startswith("\t") and s and not s.startswith(".") and not s.startswith(";")
def carriers(t):   # the VGPRs that carry spilled SGPRs in their lanes
    return set(m.group(1) for l in t if (m := re.match(r"\s+v_writelane_b32 (v\d+),", l)))
def spill_lanes(seg, car):
    return sum(1 for l in seg if ((m := re.match(r"\s+v_writelane_b32 (v\d+),", l)) or (m := re.match(r"\s+v_readlane_b32 s\d+, (v\d+),", l))) and m.group(1) in car)
def exposed_waits(seg):
    n, since = 0, None   # since: instructions issued after the last LDS load
    for l in seg:
        if not isins(l):
            continue
        op = l.split()[0]
        if op.startswith("ds_read"):
            since = 0
            continue
        if op == "s_waitcnt" and "lgkmcnt" in l and since is not None and since <= 3:
            n += 1
        if since is not None:
            since += 1
            if op == "s_waitcnt" and "lgkmcnt" in l:
                since = None
    return n
def classes(seg):
    c = Counter(l.split()[0] for l in seg if isins(l))
    g = lambda f: sum(v for k, v in c.items() if f(k))
    return (sum(c.values()), g(lambda k: "f64" in k and k.startswith("v_")), g(lambda k: k.startswith("ds_read")), g(lambda k: k.startswith("ds_write")), c.get("v_readlane_b32", 0),
            g(lambda k: "cndmask" in k), g(lambda k: k.startswith("v_mov")), g(lambda k: k.startswith("v_") and ("_u32" in k or "_i32" in k or "_b32" in k) and "cndmask" not in k and "mov" not in k and "readlane" not in k),
            c.get("s_waitcnt", 0), g(lambda k: k.startswith("s_") and k != "s_waitcnt"), g(lambda k: k.startswith("v_accvgpr")), spill_lanes(seg, CAR), exposed_waits(seg))
prod = build([])
CAR = carriers(prod)
tot = classes(prod)
print("crx_solve_kernel<%s>  production build: %d instructions (static), %s" % (tpl, tot[0], " ".join(" ".join(l.split()) for l in prod if "vgpr_count" in l or "group_segment_fixed_size:" in l or "sgpr_spill_count" in l)))
print("  SGPR-spill carriers %s: %d lane writes / reads, %d s_waitcnt in all, %d of them exposed, in the whole kernel" % (" ".join(sorted(CAR, key=lambda v: int(v[1:]))) or "(none)", tot[11], tot[8], tot[12]))
print("  (below: the build with the phase clocks in.  A clock read is a scalar memory instruction, and while one is pending an LDS wait is a full wait:")
print("   the per-phase `wait` / `xwait` figures right behind a clock read are upper bounds of the production build's)")
tr = build(["-DCRX_PHASE_CLOCKS"])
CAR = carriers(tr)
marks = [i for i, l in enumerate(tr) if "s_memtime" in l]
# the clock reads in source order: five at the head of the iteration, two around the set-up of the backward sweep, four per stage of it (once for a
# rolled stage loop, once per stage for an unrolled sweep), five behind it; with the shared sweep set-up (riccati_backward<.., SHARED>) two more behind
# the sweep, around the set-up of the next attempt, which is code of the failure path: not executed by an iteration whose first sweep succeeds
RS = 2 if len(marks) >= 18 and (len(marks) - 12) % 4 == 2 else 0
stages = (len(marks) - 12 - RS) // 4 if len(marks) >= 16 and (len(marks) - 12 - RS) % 4 == 0 else 0
names = ["(loop top)", "adjoint (KKT error)", "barrier update", "assemble", "ric: retry schedule, terminal P", "ric: lane maps, stage-invariant operands", "ric: (set-up -> first stage)"]
for s_ in range(stages):
    k = "k" if stages == 1 else "N-%d" % (s_ + 1)
    names += ["ric %s: T = P M" % k, "ric %s: H = M'T + .." % k, "ric %s: factor + update" % k, "ric %s: (-> next stage)" % k if s_ < stages - 1 or stages == 1 else "ric: sigma_0 / retry logic"]
if stages == 1:
    names += ["ric: sigma_0 / retry logic"]
if RS:
    names += ["ric: retry, terminal P of the next attempt", "ric: (retry -> first stage | out)"]
names += ["forward sweep" + (" (loop body once)" if stages == 1 else ""), "row steps", "line search (one trial)", "accept + first order"]
print("%-36s %6s %5s %5s %5s %5s %5s %5s %5s %5s %5s %5s %5s %5s" % ("phase (between clock reads)", "instr", "f64", "ds_r", "ds_w", "rdln", "cndm", "vmov", "vint", "wait", "salu", "agpr", "spill", "xwait"))
def loops(a, b):   # bodies of the loops that lie inside [a, b): (label, instructions), innermost first
    lab = {m.group(1): i for i, l in enumerate(tr[a:b], a) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    out = {}
    for i, l in enumerate(tr[a:b], a):
        m = re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in lab and lab[m.group(1)] < i:
            out[m.group(1)] = max(out.get(m.group(1), 0), sum(isins(x) for x in tr[lab[m.group(1)]:i + 1]))
    return sorted(out.items(), key=lambda kv: kv[1])
for n, (a, b) in enumerate(zip(marks[:-1], marks[1:])):
    lp = loops(a, b)
    print("%-36s %6d %5d %5d %5d %5d %5d %5d %5d %5d %5d %5d %5d %5d" % (((names[n] if n < len(names) else "?"),) + classes(tr[a + 1:b])), ("  loops: " + ", ".join("%d" % v for _, v in lp)) if lp else "")
it = classes(tr[marks[0] + 1:marks[-1]])
print("%-36s %6d %5d %5d %5d %5d %5d %5d %5d %5d %5d %5d %5d %5d" % (("iteration, first to last clock read",) + it))
