// libcrx: the TWO-WAVE unit of the solver [r6] -- outside the walk: crx_api.hip routes a launch here by itself when it leaves SIMDs idle.
//   built with    as the obstacle unit: MachineLICM off + OBS_SCHED (iterative-ilp).  Makefile, row crx_kernels_spec.o
//   holds         crx_solve_kernel<1, 12, 6, {12, 10}, SPEC = 1>: the one-obstacle, degree-6 kernel at the tuned horizons 12 and 10 -- BASELINE
//                 configs[1] and the reference's default horizon -- and nothing else
//   next          nothing: any other launch is refused
// One more wave per problem: while wave 0 factorises the reduced Hessian with the current entry of the inertia-correction schedule, wave 1 factorises
// it with the next one in a second set of work arrays (crx_kernels.hip, crx_solve_kernel: SPEC).  OPT-IN (crx_debug_speculation(1)): measured on the
// headline batch it does not pay; kept as the build VERDICT r5 asked for, with its test
// (tests/test_gpu_parity.py::test_speculating_wave_follows_the_sequential_schedule).
#include "crx_kernels.hip"

hipError_t crx_launch_solve_spec(const crx_kparams& kp, hipStream_t st) {
    if (kp.batch == 0) return hipSuccess;
    if (kp.degree != 6) return hipErrorInvalidValue;
    if (kp.N == 12) return launch_t<1, 12, 6, 12, 1>(kp, st);
    if (kp.N == 10) return launch_t<1, 12, 6, 10, 1>(kp, st);
    return hipErrorInvalidValue;
}
