// libcrx: the third MODELS unit -- crx_solve_kernel with one LTI model per problem (crx_kernels_models_plan.hip says what that is), everything the
// first two do not hold.  The walk: models_plan -> models_obs -> models_gen.
//   built with    as the general unit, whose instantiations it mirrors: MachineLICM off + GEN_FLAGS, the GENERAL BUILD of the source
//                 (CRX_TU_GENERAL: crx_kernels_gen.hip has what that gives up and why), CRX_TU_MODELS.  Makefile, row crx_kernels_models_gen.o
//   holds         every other (N, slots, exponent) the shared launch accepts, on the general instantiations (select_general, crx_kernels.hip);
//                 the planner region QP at any horizon other than 10 / 12
//   next          nothing: a launch no instantiation serves is refused
#define CRX_TU_GENERAL 1
#define CRX_TU_MODELS 1
#include "crx_kernels.hip"

struct Unit {
    template <class F>
    static bool select_inst(int nobs_template, int N, int degree, F&& f) { return select_general(nobs_template, N, degree, f); }
    static hipError_t next_launch(const crx_kparams_models&, int, hipStream_t) { return hipErrorInvalidValue; }
};
hipError_t crx_launch_solve_models_general(const crx_kparams_models& kp, int nobs_template, hipStream_t st) { return unit_launch<Unit>(kp, nobs_template, st); }
