#!/bin/bash
# A/B builds of libcrx: tools/build_variant.sh NAME "EXTRA-FLAGS" [file.hip ...]
# A thin call of the Makefile's `variant` target (car-racing_amd/csrc/Makefile), which owns the list of units and the flags of each: the named
# units (default: the two tuned units of the solver, crx_kernels_plan.hip + crx_kernels_obs.hip; the general one is crx_kernels_gen.hip) are compiled
# with their own flags + the extra ones into tools/ab/NAME/, and tools/ab/libcrx_NAME.so is linked from them plus the in-tree objects of every other
# unit -- run `make` first; the in-tree objects are not touched.  PLAN_SCHED= / OBS_SCHED= / GEN_FLAGS= / LMPC_SCHED= / NOLICM= in the environment
# override a unit flag as they do for `make` (PLAN_SCHED= : the main unit with the default scheduler).
# Select at run time: CRX_LIB=tools/ab/libcrx_NAME.so.  (*.so is git-ignored but travels to the GPU box with the snapshot.)
set -e
NAME=$1; EXTRA=$2; shift 2 || true
exec make -s -C "$(dirname "$0")/../car-racing_amd/csrc" variant NAME="$NAME" VFLAGS="$EXTRA" UNITS="${*:-crx_kernels_plan.hip crx_kernels_obs.hip}"
