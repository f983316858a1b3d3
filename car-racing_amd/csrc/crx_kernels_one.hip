// libcrx, not linked: ONE instantiation of crx_solve_kernel compiled alone, in seconds instead of minutes (tools/kernel_resources.py one NOBS NMAX DEG NFIX,
// tools/asm_census.py).  Built with -DCRX_PROBE_ONE=NOBS,NMAX,DEG,NFIX[,SPEC,QPM] and the flags of the unit that ships the instantiation (Makefile, rows
// crx_kernels_one_plan.o / crx_kernels_one_obs.o); a general or models instantiation also takes -DCRX_TU_GENERAL=1 / -DCRX_TU_MODELS=1.
#include "crx_kernels.hip"
template __global__ void crx_solve_kernel<CRX_PROBE_ONE>(const crx_solve_params);
