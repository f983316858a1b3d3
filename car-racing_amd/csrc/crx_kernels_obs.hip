// libcrx: the OBSTACLE unit of the solver -- the second of the walk plan -> obs -> gen.
//   built with    MachineLICM off + OBS_SCHED (iterative-ilp machine scheduling: +3.7 % on BASELINE configs[1], 0.991 -> 0.956 ms per 256 NLPs, +7 % on
//                 configs[3]; it costs the planner kernels 1 %, which is why they are another unit.  HISTORY.md, round 3: max-ilp, max-memory-clause,
//                 iterative-minreg and the occupancy / latency bias were measured beside it.  Same arithmetic either way: the schedule does not
//                 re-associate).  Makefile, row crx_kernels_obs.o
//   holds         the obstacle instantiations crx_solve_kernel<1..3, *> (MPC-CBF NLP, tracking NLP with CBF rows), exponent 6, at the horizons of
//                 CRX_NFIX_LIST
//   next          any other exponent (2 / 4 / 8), horizon or slot count goes to the general unit (crx_kernels_gen.hip)
#include "crx_kernels.hip"

struct Unit {
    template <class F>
    static bool select_inst(int nobs_template, int N, int degree, F&& f) {
        if (degree != 6) return false;
        switch (nobs_template) {
            case 1: return select_fixed<1, 6, CRX_NFIX_LIST>(N, f);
            case 2: return select_fixed<2, 6, CRX_NFIX_LIST>(N, f);
            case 3: return select_fixed<3, 6, CRX_NFIX_LIST>(N, f);
            default: return false;
        }
    }
    static hipError_t next_launch(const crx_kparams& kp, int nobs_template, hipStream_t st) { return crx_launch_solve_general(kp, nobs_template, st); }
    static int next_resident(int N, int nobs_template) { return crx_solve_resident_per_cu_general(N, nobs_template); }
};
hipError_t crx_launch_solve_obs(const crx_kparams& kp, int nobs_template, hipStream_t st) { return unit_launch<Unit>(kp, nobs_template, st); }
int crx_solve_resident_per_cu_obs(int N, int nobs_template) { return unit_resident<Unit>(N, nobs_template); }
