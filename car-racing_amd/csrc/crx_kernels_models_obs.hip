// libcrx: the second MODELS unit -- crx_solve_kernel with one LTI model per problem (crx_kernels_models_plan.hip says what that is), the racing
// shapes with obstacles.  The walk: models_plan -> models_obs -> models_gen.
//   built with    as the obstacle unit, whose instantiations it mirrors: MachineLICM off + OBS_SCHED (iterative-ilp), CRX_TU_MODELS.  Makefile, row
//                 crx_kernels_models_obs.o
//   holds         one obstacle slot at N = 10 / 12 and three at N = 20, exponent 6
//   next          everything else goes to the general models unit (crx_kernels_models_gen.hip)
#define CRX_TU_MODELS 1
#include "crx_kernels.hip"

struct Unit {
    template <class F>
    static bool select_inst(int nobs_template, int N, int degree, F&& f) {
        if (degree != 6) return false;
        if (nobs_template == 1) return select_fixed<1, 6, 10, 12>(N, f);
        if (nobs_template == 3) return select_fixed<3, 6, 20>(N, f);
        return false;
    }
    static hipError_t next_launch(const crx_kparams_models& kp, int nobs_template, hipStream_t st) { return crx_launch_solve_models_general(kp, nobs_template, st); }
};
hipError_t crx_launch_solve_models_obs(const crx_kparams_models& kp, int nobs_template, hipStream_t st) { return unit_launch<Unit>(kp, nobs_template, st); }
