// libcrx: the GENERAL unit of the solver [r5] -- the last of the walk plan -> obs -> gen.
//   built with    MachineLICM off + GEN_FLAGS (empty: the default machine scheduler, not iterative-ilp), and as the GENERAL BUILD of the source
//                 (CRX_TU_GENERAL, below).  Makefile, row crx_kernels_gen.o
//   holds         everything the tuned units do not: run-time horizon (every N other than those of CRX_NFIX_LIST), run-time exponent (CBF degree
//                 2 / 4 / 8), and the generic 4..6-obstacle instantiations (select_general, crx_kernels.hip)
//   next          nothing: a launch no instantiation serves is refused
// Same source as the tuned instantiations, built CONSERVATIVELY: these are the instantiations in which A/B builds of rounds 4 and 5 computed
// wrong numbers (DESIGN.md section 8 has the two causes, both in the compiler's hands: LDS accesses scheduled across a phase boundary,
// and a VGPR spill store placed in front of a loop exit's EXEC restore).  What the general build gives up (the knob defaults are stated once,
// at the head of crx_kernels.hip):
//   * no inline-assembly DPP: the sweeps broadcast with v_readlane, every hazard is the compiler's to see;
//   * nothing lane-derived is carried across the interior-point loop: the lane index is made opaque once per iteration (half the
//     register pressure of the hoisted lane maps);
//   * the plain form everywhere: no loads_first / lone_wave forms of the tuned one-obstacle instantiations (Form, crx_kernels.hip).
// Registers: static LDS, the whole unified register file (AGPR copies where 256 VGPRs do not suffice).  The other choice -- dynamic LDS +
// a floor of two waves per SIMD = 256 registers and scratch spills, -DCRX_STATIC_LDS=0 -DCRX_GEN_WAVES=2 -- was the shipped one for a few
// hours of round 5 and is where the spill-placement bug bit (tools/exec_prologue_check.py finds the pattern in the assembly; it is a
// test: every translation unit of the library must be free of it).
// Slower than the tuned path by design (correct first); every BASELINE config runs on the tuned instantiations.
#define CRX_TU_GENERAL 1
#include "crx_kernels.hip"

struct Unit {
    template <class F>
    static bool select_inst(int nobs_template, int N, int degree, F&& f) { return select_general(nobs_template, N, degree, f); }
    static hipError_t next_launch(const crx_kparams&, int, hipStream_t) { return hipErrorInvalidValue; }
    static int next_resident(int, int) { return -1; }
};
hipError_t crx_launch_solve_general(const crx_kparams& kp, int nobs_template, hipStream_t st) { return unit_launch<Unit>(kp, nobs_template, st); }
int crx_solve_resident_per_cu_general(int N, int nobs_template) { return unit_resident<Unit>(N, nobs_template); }
