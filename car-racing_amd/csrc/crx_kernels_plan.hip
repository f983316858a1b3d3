// libcrx: the MAIN unit of the solver (object crx_kernels.o) -- the head of the walk plan -> obs -> gen.
//   built with    MachineLICM off + PLAN_SCHED (max-ilp machine scheduling: +2.5 % on 4096 region QPs against the default strategy, iterative-ilp
//                 loses 1 % here; HISTORY.md, round 3).  Makefile, row crx_kernels.o
//   holds         the planner instantiations crx_solve_kernel<0, *> at the horizons of CRX_NFIX_LIST, both qp_method
//   next          a launch it has no instantiation for goes to the obstacle unit (crx_kernels_obs.hip)
//   also here     region selection (crx_select_kernel), the diagnostics of the packed wave reductions (crx_debug_reduce_kernel), their launchers, and
//                 crx_solve_lds_bytes: what the library needs once and no solver unit more than another
#include "crx_kernels.hip"

struct Unit {
    template <class F>
    static bool select_inst(int nobs_template, int N, int, F&& f) { return nobs_template == 0 && select_fixed<0, 0, CRX_NFIX_LIST>(N, f); }
    static hipError_t next_launch(const crx_kparams& kp, int nobs_template, hipStream_t st) { return crx_launch_solve_obs(kp, nobs_template, st); }
    static int next_resident(int N, int nobs_template) { return crx_solve_resident_per_cu_obs(N, nobs_template); }
};
hipError_t crx_launch_solve(const crx_kparams& kp, int nobs_template, hipStream_t st) { return unit_launch<Unit>(kp, nobs_template, st); }
int crx_solve_resident_per_cu(int N, int nobs_template) { return unit_resident<Unit>(N, nobs_template); }

// ------------------------------------------------------------------------------------------------
// region selection (planning/overtake_traj_planner.py:205-246): one wave per scenario, lanes
// over (side, stage) collision tests.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WAVE) crx_select_kernel(const crx_select_kparams sp) {
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= sp.n_scen) return;
    const int N = sp.N, V = sp.V, R = V + 1;
    const int nv = min(max(sp.n_veh[s], 0), V);   // the *_dev entry points cannot validate device-resident counts: clamp
    const double r2 = sp.veh_length * sp.veh_length + sp.veh_width * sp.veh_width;
    double best_c = INFINITY;
    int best = 0;
    for (int r = 0; r < R; r++) {
        double cst = INFINITY;
        if (r <= nv) {
            const double* Xr = sp.X + (((size_t)s * R + r) * (N + 1)) * 6;
            double hits = 0.0;
            for (int e = lane; e < 2 * (N + 1); e += WAVE) {
                const int side = e / (N + 1), j = e - side * (N + 1);
                const int v = side == 0 ? r - 1 : r;                                          // :213, :227
                if (v < 0 || v >= nv) continue;
                double os = sp.obs_s[((size_t)s * V + v) * (N + 1) + j];
                os = wrap_above(os, sp.lap_length);                                             // :216-217
                const double ds = Xr[6 * j + 4] - os;
                const double de = Xr[6 * j + 5] - sp.obs_ey[((size_t)s * V + v) * (N + 1) + j];
                if (!(ds * ds + de * de - r2 >= 0.0)) hits += 1.0;                            // :220-223
            }
            hits = wave_sum(hits);
            cst = -sp.w_prog * (Xr[6 * N + 4] - Xr[4]) + sp.w_coll * hits;                    // :209
            if (sp.old_flag[s] >= 0 && sp.old_flag[s] != r) cst += sp.w_switch;               // :238-243
            if (cst < best_c) { best_c = cst; best = r; }                                     // first arg-min :244
        }
        if (lane == 0) sp.sel_cost[(size_t)s * R + r] = cst;
    }
    if (lane == 0) sp.flag[s] = best;
    const double* Xb = sp.X + (((size_t)s * R + best) * (N + 1)) * 6;
    for (int e = lane; e < (N + 1) * 6; e += WAVE) sp.best_X[(size_t)s * (N + 1) * 6 + e] = Xb[e];
}

size_t crx_solve_lds_bytes(int N, int nobs_template) { return layout_bytes(N, nobs_template); }

hipError_t crx_launch_select(const crx_select_kparams& sp, hipStream_t st) {
    if (sp.n_scen == 0) return hipSuccess;
    hipLaunchKernelGGL(crx_select_kernel, dim3(sp.n_scen), dim3(WAVE), 0, st, sp);
    return hipGetLastError();
}

// diagnostics (crx_debug_wave_reduce, not in crx.h): the packed wave reductions of crx_wave.h on four 64-lane inputs.
// out [16 + 3 * 64]: out[0..3] wave_sum4, [4..7] wave_max4, [8..9] wave_sum2 of inputs 0 and 1, [10..11] wave_max2 of inputs 2 and 3,
// [12..15] the single-value reductions (sum of 0, max of 1, min of 2, product of the mantissas of 3).
__global__ void __launch_bounds__(WAVE) crx_debug_reduce_kernel(const double* in, double* out) {
    const int lane = threadIdx.x;
    double a = in[lane], b = in[64 + lane], c = in[128 + lane], d = in[192 + lane];
    double s0 = a, s1 = b, s2 = c, s3 = d;
    wave_sum4(s0, s1, s2, s3);
    double m0 = a, m1 = b, m2 = c, m3 = d;
    wave_max4(m0, m1, m2, m3);
    double p0 = a, p1 = b;
    wave_sum2(p0, p1);
    double q0 = c, q1 = d;
    wave_max2(q0, q1);
    int ex;
    const double r0 = wave_sum(a), r1 = wave_max(b), r2 = wave_min(c), r3 = wave_prod(frexp(fabs(d) + 1.0, &ex));
    if (lane == 0) {
        out[0] = s0; out[1] = s1; out[2] = s2; out[3] = s3; out[4] = m0; out[5] = m1; out[6] = m2; out[7] = m3;
        out[8] = p0; out[9] = p1; out[10] = q0; out[11] = q1; out[12] = r0; out[13] = r1; out[14] = r2; out[15] = r3;
    }
    // [r4] row_dot (v_fmac_f64_dpp row_newbcast): out[16 + lane] = c + sum_{i<7} m_i * (lane i of a's 16-lane row), m_i = (i + 1) b + d, under
    // full EXEC; out[80 + lane] = the same with terms 3 .. 9 inside an `if (lane < 10)` region (the sweeps' predication; NaN elsewhere);
    // out[144 + lane] = a three-term dot product of lanes 7 .. 9 whose x is the value just accumulated (the forward sweep's input term)
    double m[7];
#pragma unroll
    for (int i = 0; i < 7; i++) m[i] = (double)(i + 1) * b + d;
    out[16 + lane] = row_dot<7, 0>(a, m, c);
    double masked = __longlong_as_double(0x7ff8000000000000LL), chained = masked;
    if (lane < 10) {
        masked = row_dot<7, 3>(a, m, c);
        const double first = row_dot<7, 0>(a, m, c);
        chained = row_dot<3, 7>(first, m, first);
    }
    out[80 + lane] = masked;
    out[144 + lane] = chained;
}

hipError_t crx_launch_debug_reduce(const double* in, double* out, hipStream_t st) {
    hipLaunchKernelGGL(crx_debug_reduce_kernel, dim3(1), dim3(WAVE), 0, st, in, out);
    return hipGetLastError();
}
