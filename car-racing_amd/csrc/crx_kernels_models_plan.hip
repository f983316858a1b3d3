// libcrx: the first MODELS unit -- crx_solve_kernel with ONE LTI MODEL PER PROBLEM (MPC-CBF NLP, tracking NLP: crx_cbf_solve_models*; planner region
// QP: crx_planner_solve_models*), the head of the walk models_plan -> models_obs -> models_gen.  Same source as the shared-model instantiations
// (crx_kernels.hip), whose kernels take the model in crx_kparams; under CRX_TU_MODELS the kernel takes crx_kparams_models and problem b reads A, B
// from model_A[36 b ..], model_B[12 b ..] and its reach tables from model_reach -- in set-up only: the model matrix M, crash_search (which reads M
// back) and the slack bounds.  The interior-point loop is the shared kernels' loop.  Each of the three units is built with the flags of the
// shared-model unit whose instantiations it mirrors.  The two-wave kernels have no such twin.
//   built with    as the main unit: MachineLICM off + PLAN_SCHED (max-ilp), CRX_TU_MODELS.  Makefile, row crx_kernels_models_plan.o
//   holds         zero obstacle slots at N = 10 / 12: the mpc_lti form of the CBF NLP, and the planner region QP (mode 0), whose reachability screen
//                 reads problem b's table from model_reach, laid out for it by crx_planner_reach_kernel below
//   next          launches with obstacle slots go to crx_kernels_models_obs.hip
//   also here     crx_cbf_reach_kernel and crx_planner_reach_kernel with their launchers: two small kernels that fill model_reach
#define CRX_TU_MODELS 1
#include "crx_kernels.hip"

struct Unit {
    template <class F>
    static bool select_inst(int nobs_template, int N, int, F&& f) { return nobs_template == 0 && select_fixed<0, 0, 10, 12>(N, f); }
    static hipError_t next_launch(const crx_kparams_models& kp, int nobs_template, hipStream_t st) { return crx_launch_solve_models_obs(kp, nobs_template, st); }
};
hipError_t crx_launch_solve_models(const crx_kparams_models& kp, int nobs_template, hipStream_t st) { return unit_launch<Unit>(kp, nobs_template, st); }

// (lives in this unit, not beside crx_cbfprep_kernel, so that no code object of the shared-model library changes)
// crx_cbf_reach_kernel: the reach tables of the CBF NLP for one LTI model per problem (crx_cbf_models_reach_dev).  One thread per (problem, row):
// r = 0 restates reach_bound (crx_api.hip) for state row 4 (s), r = 1 for row 5 (ey), stages 0 .. N, entries past N zero, into
// model_reach [batch][2][CRX_MAX_N + 1].  Same operations in the same order as the host function, every product and sum rounded on its own
// (contraction off for the whole body; HIP's __dmul_rn / __dadd_rn are plain operators and would be fused), so a copy of the descriptor's
// model gives the descriptor's table bit for bit.
__global__ void __launch_bounds__(256) crx_cbf_reach_kernel(int N, int batch, double delta_max, double a_max, const double* model_A,
                                                            const double* model_B, double* model_reach) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * batch) return;
    const int b = t >> 1, r = t & 1;
    const double* A = model_A + (size_t)36 * b;
    const double* B = model_B + (size_t)12 * b;
    double* gain = model_reach + ((size_t)2 * b + r) * (CRX_MAX_N + 1);
    double w[6] = {0, 0, 0, 0, r ? 0.0 : 1.0, r ? 1.0 : 0.0}, acc = 0.0;
    gain[0] = 0.0;
    for (int j = 1; j <= N; j++) {
        double v0 = 0.0, v1 = 0.0, wn[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 6; i++) { v0 += w[i] * B[i * 2]; v1 += w[i] * B[i * 2 + 1]; }
        acc += fabs(v0) * delta_max + fabs(v1) * a_max;
        gain[j] = acc;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int i = 0; i < 6; i++) wn[a] += w[i] * A[i * 6 + a];
#pragma unroll
        for (int a = 0; a < 6; a++) w[a] = wn[a];
    }
    for (int j = N + 1; j <= CRX_MAX_N; j++) gain[j] = 0.0;
}

hipError_t crx_launch_cbf_reach(int N, int batch, double delta_max, double a_max, const double* model_A, const double* model_B, double* model_reach,
                                hipStream_t st) {
    if (batch == 0) return hipSuccess;
    hipLaunchKernelGGL(crx_cbf_reach_kernel, dim3((2 * batch + 255) / 256), dim3(256), 0, st, N, batch, delta_max, a_max, model_A, model_B, model_reach);
    return hipGetLastError();
}

// crx_planner_reach_kernel: the reachability-screen table of the planner region QP for one LTI model per problem (crx_planner_models_reach_dev;
// here for the reason above).  One thread per problem restates reach_bound(A, B, delta_max, a_max, 5, N - 1, gain, rows) of crx_api.hip, same
// operations in the same order with contraction off, into model_reach [batch][CRX_MAX_N][7]: stage j holds rows[j] = e_ey' A^j (6 doubles), then
// gain[j] -- the seven doubles lane j of the solver's screen reads.  Stages j >= N are zero.  A copy of the descriptor's model gives the
// descriptor's reach_row / reach_gain bit for bit.
__global__ void __launch_bounds__(256) crx_planner_reach_kernel(int N, int batch, double delta_max, double a_max, const double* model_A,
                                                                const double* model_B, double* model_reach) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const double* A = model_A + (size_t)36 * b;
    const double* B = model_B + (size_t)12 * b;
    double* tab = model_reach + (size_t)CRX_MAX_N * 7 * b;
    double w[6] = {0, 0, 0, 0, 0, 1.0}, acc = 0.0;
#pragma unroll
    for (int a = 0; a < 6; a++) tab[a] = w[a];
    tab[6] = 0.0;
    for (int j = 1; j < N; j++) {
        double v0 = 0.0, v1 = 0.0, wn[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 6; i++) { v0 += w[i] * B[i * 2]; v1 += w[i] * B[i * 2 + 1]; }
        acc += fabs(v0) * delta_max + fabs(v1) * a_max;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int i = 0; i < 6; i++) wn[a] += w[i] * A[i * 6 + a];
#pragma unroll
        for (int a = 0; a < 6; a++) { w[a] = wn[a]; tab[j * 7 + a] = wn[a]; }
        tab[j * 7 + 6] = acc;
    }
    for (int e = N * 7; e < CRX_MAX_N * 7; e++) tab[e] = 0.0;
}

hipError_t crx_launch_planner_reach(int N, int batch, double delta_max, double a_max, const double* model_A, const double* model_B,
                                    double* model_reach, hipStream_t st) {
    if (batch == 0) return hipSuccess;
    hipLaunchKernelGGL(crx_planner_reach_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, N, batch, delta_max, a_max, model_A, model_B, model_reach);
    return hipGetLastError();
}
