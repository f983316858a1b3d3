#!/bin/bash
# A/B builds of the solver kernels whose code generation differs most; every variant must pass the parity tests on the GPU
# (ADVICE r3 / VERDICT r4 item 1: two A/B builds of round 4 computed wrong numbers -- DESIGN.md section 8).  Build here (no GPU needed), then on
# the GPU:  bash tools/gpu_pass.sh TAG gen:g000 gen:g001 ... gen:g111 suite:fenceonly suite:opaqueall suite:nodpp
# [r5] The GENERAL instantiations (csrc/crx_kernels_gen.hip: run-time horizon / exponent, 4..6 obstacles) over the full 2^3 matrix of the
# three flags whose combination failed in round 4: gSDM with S = static LDS (+ no register floor: the AGPR-parking build), D = inline-assembly
# DPP dot products, M = masked sweeps (the shipped unit is g101: static LDS + AGPR copies, v_readlane, masked sweeps).  Every cell is first
# passed through tools/exec_prologue_check.py (a spill store in front of an EXEC restore: the compiler bug of DESIGN.md section 8); the S = 0 cells
# spill to scratch and are where it appears.
# Units are named by their source files (car-racing_amd/csrc/Makefile has the table; tools/build_variant.sh is a thin call of its `variant` target).
# Tuned units: fenceonly = SYNC() as up to 0.2.1 (fence without the wave barrier), opaqueall / nodpp as in round 4.
cd "$(dirname "$0")/.."
rm -rf tools/ab/g[01][01][01] tools/ab/libcrx_g[01][01][01].so
for S in 0 1; do for D in 0 1; do
  for M in 0 1; do
    W=2; [ $S = 1 ] && W=0
    bash tools/build_variant.sh g$S$D$M "-DCRX_STATIC_LDS=$S -DCRX_GEN_WAVES=$W -DCRX_ROWDPP=$D -DCRX_SWEEP_MASK=$M" crx_kernels_gen.hip > /dev/null &
  done; wait
done; done
for c in 000 001 010 011 100 101 110 111; do
  S=${c:0:1}; D=${c:1:1}; M=${c:2:1}; W=2; [ $S = 1 ] && W=0
  echo "g$c: $(python tools/exec_prologue_check.py tools/ab/libcrx_g$c.so | tail -1)"     # [r6] on the code objects of the variant itself
done | tee tools/ab/exec_prologue_matrix.txt
# fenceonly: EVERY unit whose source, or the kernel text it includes (crx_kernels.hip, crx_path_qp.h), uses SYNC() -- grep -l 'SYNC()' csrc
FENCE_UNITS="crx_kernels_plan.hip crx_kernels_obs.hip crx_kernels_spec.hip crx_kernels_gen.hip crx_kernels_models_plan.hip crx_kernels_models_obs.hip"
FENCE_UNITS="$FENCE_UNITS crx_kernels_models_gen.hip crx_lmpc.hip crx_lmpcprep.hip crx_path.hip crx_pathplan.hip crx_ilqr.hip crx_lqr.hip crx_sysid.hip crx_debug_wave.hip"
bash tools/build_variant.sh fenceonly "-DCRX_SYNC_FENCE_ONLY" $FENCE_UNITS > /dev/null &
bash tools/build_variant.sh opaqueall "-DCRX_OPAQUE_LANE=2" crx_kernels_obs.hip > /dev/null &
# (nodpp runs the lone-wave kernels' inertia retries outside the sweep function: riccati_backward<.., SHARED> is written for the register-resident
# (P | p), which needs the DPP form, and crx_solve_kernel takes it only where ROWDPP holds)
bash tools/build_variant.sh nodpp "-DCRX_ROWDPP=0" crx_kernels_plan.hip crx_kernels_obs.hip > /dev/null &
wait
ls -la tools/ab/*.so
# every library of the list must be whole: it loads (needs no GPU) -- a variant that lacks a unit of the link line fails here with an undefined symbol
for n in g000 g001 g010 g011 g100 g101 g110 g111 fenceonly opaqueall nodpp; do
  python -c "import ctypes, sys; ctypes.CDLL(sys.argv[1]); print('loads', sys.argv[1])" tools/ab/libcrx_$n.so || exit 1
done
