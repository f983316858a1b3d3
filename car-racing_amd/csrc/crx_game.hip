// crx_game.hip -- the racing game's bookkeeping between the solver launches:
//   crx_game_traffic_kernel   the scripted cars at their own clock and their predictions      utils/base.py:847-890, :795-819
//   crx_game_masks_kernel     which branch a race takes this step, as the masks of the masked launches      utils/base.py:463-467
//   crx_game_commit_kernel    the applied input and the learning MPC's hand-over of its plan      control/control.py:726-728, utils/base.py:504-515, :546-551
//   crx_game_log_kernel       the simulator's lap log and the races that completed a lap      utils/base.py:780-819, racing/offboard.py:114-131
// the seed laps in front of the learning MPC (include/crx.h, "Seed laps" S1-S6):
//   crx_seed_commit_kernel, crx_seed_log_kernel      each car's PID lap, then its MPC-LTI lap, logged into its own safe set      tests/auto_racing_game_test.py:48-73
// the commit of a mixed field (include/crx.h, "Mixed fields"):
//   crx_mixed_commit_kernel      each car's input from its own controller's law: PID, LQR, stage 0 of its NLP or iLQR plan, or nothing      racing/offboard.py:14-45
// and what the closed loops are run for (include/crx.h, "Race statistics"):
//   crx_race_stats_reset_kernel, crx_race_stats_kernel, crx_race_stats_summary_kernel      per-car outcomes, one launch per sample; the batch summary
//
// ------------------------------------------------------------------------------------------------
// Device-resident racing-game loop (crx.montecarlo.GameLaps): the bookkeeping of
// LMPCRacingGame.calc_input (utils/base.py:456-583) and of the simulator (racing/offboard.py:114-131, base.py:780-819)
// between the solver launches, one thread per race (or per race and car).  Round 2 did this with ~40 element-wise torch
// launches per control step; these four kernels are the same assignments in the same order.
// ------------------------------------------------------------------------------------------------
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "crx_kparams.h"
#include "crx_num.h"

// scripted cars at their own clock t (NoDynamicsModel, base.py:847-890): s = v t + s0 wrapped once past the line like
// update_memory keeps it (base.py:795-819), predictions v (t + j dt) + s0 unwrapped (get_trajectory_nsteps: quirk Q6)
__global__ void __launch_bounds__(256) crx_game_traffic_kernel(const crx_game_kparams gp) {
#pragma clang fp contract(off)   // multiply, then add, as the element-wise formulation this replaces did (and NumPy does)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= gp.batch * gp.n_cars) return;
    const double v = gp.car_v[i], s0 = gp.car_s0[i], ey = gp.car_ey[i], L = gp.lap_length;
    const double s_now = v * gp.t + s0;
    double* x = gp.veh_xcurv + (size_t)6 * i;
    x[0] = v; x[1] = 0.0; x[2] = 0.0; x[3] = 0.0;
    x[4] = s_now - L * fmax(ceil(s_now / L) - 1.0, 0.0);
    x[5] = ey;
    const int N1 = gp.Np + 1;
    for (int j = 0; j < N1; j++) {
        gp.pred_s[(size_t)i * N1 + j] = v * (gp.t + (double)j * gp.dt) + s0;
        gp.pred_ey[(size_t)i * N1 + j] = ey + 0.0 * ((double)j * gp.dt);
    }
}

// which branch a race takes this step (utils/base.py:463-467: vehicles of interest -> overtake planner + tracking NLP, none ->
// learning MPC), as the `active` masks of the masked launches
__global__ void __launch_bounds__(256) crx_game_masks_kernel(const crx_game_kparams gp) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= gp.batch) return;
    const int ot = gp.n_veh[b] > 0 ? 1 : 0;
    gp.m_overtake[b] = ot;
    gp.m_lmpc[b] = 1 - ot;
    if (gp.overflow_seen) gp.overflow_seen[b] += gp.overflow[b];
}

// after the solves: the input the race applies, the learning MPC's hand-over of its plan (u_old, linearisation points shifted
// by one stage with the last one repeated: control.py:726-728 / utils/base.py:504-515), the step counter of add_point and the
// direction flag (utils/base.py:546-551) -- each from the branch the race is in; the other branch's state is left alone
__global__ void __launch_bounds__(256) crx_game_commit_kernel(const crx_game_kparams gp) {
    // one thread per (race, element of the plan hand-over): E = 6 (N + 1) + 2 N elements; thread 0 of a race also does its scalars
    const int N = gp.N, EX = 6 * (N + 1), E = EX + 2 * N;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)gp.batch * E) return;
    const int b = (int)(i / E), e = (int)(i - (size_t)b * E);
    const bool ot = gp.overtake && gp.overtake[b] != 0;
    const double* Ul = gp.U_lmpc + (size_t)b * N * 2;
    const double* Xl = gp.X_lmpc + (size_t)b * (N + 1) * 6;
    if (e == 0) {
        const double u0 = ot ? gp.U_track[(size_t)b * gp.Np * 2] : Ul[0], u1 = ot ? gp.U_track[(size_t)b * gp.Np * 2 + 1] : Ul[1];
        gp.u[2 * b] = u0; gp.u[2 * b + 1] = u1;
        gp.u_prev[2 * b] = gp.u_old[2 * b]; gp.u_prev[2 * b + 1] = gp.u_old[2 * b + 1];
        gp.addpoint_step[b] = ot ? -(1 << 20) : gp.step_no[b];
        if (gp.old_flag) gp.old_flag[b] = ot ? gp.flag[b] : -1;
        if (!ot) { gp.u_old[2 * b] = Ul[0]; gp.u_old[2 * b + 1] = Ul[1]; gp.step_no[b] += 1; }
    }
    if (ot) return;
    if (e < EX) {                       // lin_points[k] <- X[k + 1], the last stage repeated
        const int k = e / 6, c = e - 6 * k, ks = k < N ? k + 1 : N;
        gp.lin_points[(size_t)b * EX + e] = Xl[6 * ks + c];
    } else {                            // lin_input[k] <- U[k + 1], the last stage repeated
        const int q = e - EX, k = q >> 1, c = q & 1, ks = k < N - 1 ? k + 1 : N - 1;
        gp.lin_input[(size_t)b * 2 * N + q] = Ul[2 * ks + c];
    }
}

// after the plant: the lap log the simulator keeps (ModelBase.update_memory: the new state -- the one that crossed the line
// with its s unwrapped -- and the applied input) and which races have just completed a lap (-> crx_lmpc_addtraj_dev).
// One car's assignments, shared by crx_game_log_kernel and crx_seed_log_kernel (include/crx.h S5); returns `crossed`
__device__ __forceinline__ int game_log_car(int b, int P, double lap_length, const double* xcurv, const double* u, const int32_t* laps,
                                            int32_t* laps_prev, int32_t* crossed, double* log_x, double* log_u, int32_t* n_log) {
    const int cr = laps[b] > laps_prev[b] ? 1 : 0;
    laps_prev[b] = laps[b];
    crossed[b] = cr;
    const int n = n_log[b];
    const int ix = n < P - 1 ? n : P - 1;
    int iu = n - 1; iu = iu < 0 ? 0 : (iu > P - 1 ? P - 1 : iu);
    const double* x = xcurv + (size_t)6 * b;
    double* lx = log_x + ((size_t)b * P + ix) * 6;
    for (int c = 0; c < 6; c++) lx[c] = x[c];
    lx[4] = x[4] + lap_length * (double)cr;
    double* lu = log_u + ((size_t)b * P + iu) * 2;
    lu[0] = u[2 * b]; lu[1] = u[2 * b + 1];
    n_log[b] = n + 1;
    return cr;
}

__global__ void __launch_bounds__(256) crx_game_log_kernel(const crx_game_kparams gp) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= gp.batch) return;
    game_log_car(b, gp.n_points, gp.lap_length, gp.xcurv, gp.u, gp.laps, gp.laps_prev, gp.crossed, gp.log_x, gp.log_u, gp.n_log);
}

// ------------------------------------------------------------------------------------------------
// Seed laps (crx.montecarlo.SeedLaps, include/crx.h S1-S6): every car drives its own PID lap and its own MPC-LTI lap
// (tests/auto_racing_game_test.py:48-73) and crx_lmpc_addtraj_dev turns both into the car's own safe set.  The cars finish at
// different steps, so each carries its phase: 0 PID lap, 1 MPC-LTI lap, 2 seeded, 3 failed.  One thread per car; thread b touches
// car b's elements only.
// ------------------------------------------------------------------------------------------------
// after the solver launch, before the plant: the input the car applies in the lap it is in.  The PID law is restated here, not shared with
// pid_log_kernel (crx_sysid.hip): HIP's __dmul_rn / __dsub_rn are plain operators, so that kernel's law is compiled WITH contraction
// (one of the two products fuses into the subtraction: a v_fmac_f64) and is up to an ulp from NumPy's; giving it this form would change crx_pid_log_dev's bits
__global__ void __launch_bounds__(256) crx_seed_commit_kernel(const crx_seed_kparams sp) {
#pragma clang fp contract(off)   // every operation rounded on its own: tests/seed_model.py reproduces the bits in NumPy
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= sp.batch) return;
    const int ph = sp.phase[b];
    double u0 = 0.0, u1 = 0.0;                                       // S3: a seeded or failed car applies nothing
    if (ph == 0) {                                                   // S1: control.pid (control/control.py:15-25)
        const double* x = sp.x + (size_t)6 * b;
        u0 = -0.6 * (x[5] - sp.eyt[b]) - 0.9 * x[3];
        u1 = 1.5 * (sp.vt[b] - x[0]);
    } else if (ph == 1) {                                            // S2: u_0 of the MPC-LTI plan; a failed solve is flagged, its last iterate applied
        u0 = sp.U_mpc[(size_t)b * sp.u_stride]; u1 = sp.U_mpc[(size_t)b * sp.u_stride + 1];
        if (sp.mpc_status[b] != CRX_CONVERGED) sp.seed_status[b] |= CRX_SEED_MPC_FAILED;
    }
    sp.u[2 * b] = u0; sp.u[2 * b + 1] = u1;
}

// after the plant, before crx_lmpc_addtraj_dev: a seeded car stands where it was handed over, a driving car logs the step as the
// racing game does and moves on to its next lap when it crossed the line
__global__ void __launch_bounds__(256) crx_seed_log_kernel(const crx_seed_kparams sp) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= sp.batch) return;
    int ph = sp.phase[b];
    if (ph >= 2) {                                                   // S4: frozen
        for (int c = 0; c < 6; c++) {
            sp.xcurv[(size_t)6 * b + c] = sp.xcurv_prev[(size_t)6 * b + c];
            sp.xglob[(size_t)6 * b + c] = sp.xglob_prev[(size_t)6 * b + c];
        }
        sp.laps[b] = sp.laps_prev[b];
        sp.crossed[b] = 0;
        return;
    }
    const int cr = game_log_car(b, sp.n_points, sp.lap_length, sp.xcurv, sp.u, sp.laps, sp.laps_prev, sp.crossed, sp.log_x, sp.log_u, sp.n_log);   // S5
    if (cr) {                                                        // S6
        ph += 1;
    } else if (sp.n_log[b] == sp.n_points) {                         // no row is left for the next state
        ph = 3;
        sp.seed_status[b] |= CRX_SEED_LOG_FULL;
    }
    sp.phase[b] = ph;
    sp.m_mpc[b] = ph == 1 ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// Mixed fields (crx.montecarlo.MixedRaces, include/crx.h "Mixed fields"): after the solver launches, before the plant, the input each car
// applies under its OWN controller.  One thread per car; thread b touches car b's elements only.  The policy code is compared, never
// used as an index; a code out of range, NONE, and a car whose family's arrays are not given apply zero and report CRX_SKIPPED.
// The PID law is crx_seed_commit_kernel's, the LQR sum crx_lqr_step_kernel's order (c = 0 .. 5) without its contraction.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) crx_mixed_commit_kernel(const crx_mixed_commit_kparams cp) {
#pragma clang fp contract(off)   // every operation rounded on its own: tests/mixed_model.py reproduces the bits in NumPy
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= cp.batch) return;
    const int pol = cp.policy[b];
    const double* x = cp.x + (size_t)6 * b;
    double u0 = 0.0, u1 = 0.0;
    int st = CRX_SKIPPED;
    if (pol == CRX_POLICY_PID && cp.vt) {                             // control.pid (control/control.py:15-25)
        u0 = -0.6 * (x[5] - cp.eyt[b]) - 0.9 * x[3];
        u1 = 1.5 * (cp.vt[b] - x[0]);
        st = CRX_CONVERGED;
    } else if (pol == CRX_POLICY_LQR && cp.K) {                       // control.lqr: u = -K (x - xt)
        const double* K = cp.K + (size_t)12 * b;
        const double* xt = cp.xt + (size_t)6 * b;
        double v0 = 0.0, v1 = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            const double dc = x[c] - xt[c];
            v0 += K[c] * dc;
            v1 += K[6 + c] * dc;
        }
        u0 = -v0; u1 = -v1;
        st = CRX_CONVERGED;
    } else if ((pol == CRX_POLICY_MPC_LTI || pol == CRX_POLICY_MPCCBF) && cp.U_nlp) {   // u_0 of the plan; a failed solve's last iterate (control.py:600-603)
        u0 = cp.U_nlp[(size_t)b * cp.nlp_stride]; u1 = cp.U_nlp[(size_t)b * cp.nlp_stride + 1];
        st = cp.nlp_status[b];
    } else if (pol == CRX_POLICY_ILQR && cp.U_ilqr) {
        u0 = cp.U_ilqr[(size_t)b * cp.ilqr_stride]; u1 = cp.U_ilqr[(size_t)b * cp.ilqr_stride + 1];
        st = cp.ilqr_status[b];
    }
    cp.u[2 * b] = u0; cp.u[2 * b + 1] = u1;
    cp.ctrl_status[b] = st;
}

// ------------------------------------------------------------------------------------------------
// Race statistics (crx.montecarlo.RaceStats, include/crx.h S1-S4): what the closed loops are run for, accumulated per car.  The
// outcome arithmetic used to be ~15 element-wise torch launches per step in tools/multi_tests.py; here one sample of every car is one
// launch, one thread per car, state field-major ([field][batch]) so that a wave's accesses coalesce.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) crx_race_stats_reset_kernel(const crx_stats_kparams sp) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= sp.batch) return;
    const size_t Bn = (size_t)sp.batch;
    int32_t* si = sp.stat_i + b;
    double* sd = sp.stat_d + b;
    for (int f = 0; f < CRX_STATS_NI; f++) si[f * Bn] = 0;
    si[CRX_STATS_I_NONFINITE_STEP * Bn] = -1; si[CRX_STATS_I_OFF_STEP * Bn] = -1; si[CRX_STATS_I_CONTACT_STEP * Bn] = -1;
    si[CRX_STATS_I_LAPS_PREV * Bn] = sp.laps[b];
    for (int k = 0; k < CRX_STATS_MAX_LAPS; k++) si[(CRX_STATS_I_LAP_STEP + k) * Bn] = -1;
    sd[CRX_STATS_D_MIN_CLEAR * Bn] = INFINITY; sd[CRX_STATS_D_EY_MAX * Bn] = 0.0;
    sd[CRX_STATS_D_SUM_EY2 * Bn] = 0.0; sd[CRX_STATS_D_SUM_DV2 * Bn] = 0.0;
    for (int j = 0; j < sp.d.n_opp_max; j++) sd[(CRX_STATS_D_DS_PREV + j) * Bn] = NAN;
}

// one sample (crx_race_stats_step.h, the kernel's text, once per lap-length source): crx_race_stats_kernel folds every car by the descriptor's
// lap length; crx_race_stats_laps_kernel (crx_race_stats_laps_dev) folds car b by lap_lengths[b] -- the cars of a launch on tracks of their
// own -- and counts a car whose lap length is not positive and finite as a non-finite row
#define CRX_STATS_KERNEL crx_race_stats_kernel
#define CRX_STATS_KPARAMS crx_stats_kparams
#define CRX_STATS_LAP(sp, b) d.lap_length
#define CRX_STATS_LAP_CHECK(finite, L)
#include "crx_race_stats_step.h"
#undef CRX_STATS_KERNEL
#undef CRX_STATS_KPARAMS
#undef CRX_STATS_LAP
#undef CRX_STATS_LAP_CHECK

#define CRX_STATS_KERNEL crx_race_stats_laps_kernel
#define CRX_STATS_KPARAMS crx_stats_kparams_laps
#define CRX_STATS_LAP(sp, b) sp.lap_lengths[b]
#define CRX_STATS_LAP_CHECK(finite, L) finite = finite && L > 0.0 && isfinite(L);
#include "crx_race_stats_step.h"
#undef CRX_STATS_KERNEL
#undef CRX_STATS_KPARAMS
#undef CRX_STATS_LAP
#undef CRX_STATS_LAP_CHECK

// the cars of one group to one record: a workgroup per group, every thread strides over the batch, then one tree per field over LDS.
// Integer sums, minima and maxima only, so the record does not depend on the order of the cars
enum StatsOp { STATS_ADD, STATS_MIN, STATS_MAX };
template <StatsOp OP, typename T>
__device__ T stats_block_reduce(T v, T* red) {
    __syncthreads();   // the previous field's tree has been read
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const T o = red[threadIdx.x + w], m = red[threadIdx.x];
            red[threadIdx.x] = OP == STATS_ADD ? m + o : (OP == STATS_MIN ? (o < m ? o : m) : (o > m ? o : m));
        }
        __syncthreads();
    }
    return red[0];
}

__global__ void __launch_bounds__(256) crx_race_stats_summary_kernel(const crx_stats_kparams sp) {
    __shared__ long long red_i[256];
    __shared__ double red_d[256];
    const int g = blockIdx.x;
    const size_t Bn = (size_t)sp.batch;
    long long acc[CRX_STATS_SUM_NI];
    for (int f = 0; f < CRX_STATS_SUM_NI; f++) acc[f] = 0;
    acc[CRX_STATS_SUM_LAP1_MIN] = acc[CRX_STATS_SUM_LAP2_MIN] = INT64_MAX;
    acc[CRX_STATS_SUM_LAP1_MAX] = acc[CRX_STATS_SUM_LAP2_MAX] = -1;
    double min_clear = INFINITY, ey_max = 0.0;
    for (int b = threadIdx.x; b < sp.batch; b += blockDim.x) {
        if (sp.group && sp.group[b] != g) continue;
        const int32_t* si = sp.stat_i + b;
        const bool nf = si[CRX_STATS_I_NONFINITE_STEP * Bn] >= 0, off = si[CRX_STATS_I_OFF_STEP * Bn] >= 0;
        const bool hit = si[CRX_STATS_I_CONTACT_STEP * Bn] >= 0;
        acc[CRX_STATS_SUM_CARS] += 1;
        acc[CRX_STATS_SUM_NONFINITE] += nf; acc[CRX_STATS_SUM_OFF] += off; acc[CRX_STATS_SUM_CONTACT] += hit;
        acc[CRX_STATS_SUM_CLEAN] += !(nf || off || hit);
        const int nl = si[CRX_STATS_I_N_LAPS * Bn];
        for (int k = 0; k <= CRX_STATS_MAX_LAPS; k++)   // (no run-time index into acc: it stays in registers)
            acc[CRX_STATS_SUM_LAPS_HIST + k] += (nl < CRX_STATS_MAX_LAPS ? nl : CRX_STATS_MAX_LAPS) == k;
        acc[CRX_STATS_SUM_PASSES] += si[CRX_STATS_I_PASSES * Bn];
        acc[CRX_STATS_SUM_PASSED] += si[CRX_STATS_I_PASSED * Bn];
        acc[CRX_STATS_SUM_FLAG_SAMPLES] += si[CRX_STATS_I_FLAG_SAMPLES * Bn];
        acc[CRX_STATS_SUM_N_SAMPLES] += si[CRX_STATS_I_N_SAMPLES * Bn];
        const long long t0 = si[CRX_STATS_I_LAP_STEP * Bn], t1 = si[(CRX_STATS_I_LAP_STEP + 1) * Bn];
        if (t0 >= 0) {
            acc[CRX_STATS_SUM_LAP1_SUM] += t0; acc[CRX_STATS_SUM_LAP1_COUNT] += 1;
            if (t0 < acc[CRX_STATS_SUM_LAP1_MIN]) acc[CRX_STATS_SUM_LAP1_MIN] = t0;
            if (t0 > acc[CRX_STATS_SUM_LAP1_MAX]) acc[CRX_STATS_SUM_LAP1_MAX] = t0;
        }
        if (t0 >= 0 && t1 >= 0) {
            const long long t2 = t1 - t0;
            acc[CRX_STATS_SUM_LAP2_SUM] += t2; acc[CRX_STATS_SUM_LAP2_COUNT] += 1;
            if (t2 < acc[CRX_STATS_SUM_LAP2_MIN]) acc[CRX_STATS_SUM_LAP2_MIN] = t2;
            if (t2 > acc[CRX_STATS_SUM_LAP2_MAX]) acc[CRX_STATS_SUM_LAP2_MAX] = t2;
        }
        const double mc = sp.stat_d[CRX_STATS_D_MIN_CLEAR * Bn + b], em = sp.stat_d[CRX_STATS_D_EY_MAX * Bn + b];
        min_clear = mc < min_clear ? mc : min_clear;
        ey_max = em > ey_max ? em : ey_max;
    }
    long long* out = sp.sum_i + (size_t)g * CRX_STATS_SUM_NI;
#pragma unroll
    for (int f = 0; f < CRX_STATS_SUM_NI; f++) {
        const bool lo = f == CRX_STATS_SUM_LAP1_MIN || f == CRX_STATS_SUM_LAP2_MIN, hi = f == CRX_STATS_SUM_LAP1_MAX || f == CRX_STATS_SUM_LAP2_MAX;
        long long v = lo ? stats_block_reduce<STATS_MIN>(acc[f], red_i) : (hi ? stats_block_reduce<STATS_MAX>(acc[f], red_i) : stats_block_reduce<STATS_ADD>(acc[f], red_i));
        if (lo && v == INT64_MAX) v = -1;   // no car of the group has that lap
        if (threadIdx.x == 0) out[f] = v;
    }
    const double mc = stats_block_reduce<STATS_MIN>(min_clear, red_d), em = stats_block_reduce<STATS_MAX>(ey_max, red_d);
    if (threadIdx.x == 0) {
        sp.sum_d[(size_t)g * CRX_STATS_SUM_ND + CRX_STATS_SUM_D_MIN_CLEAR] = mc;
        sp.sum_d[(size_t)g * CRX_STATS_SUM_ND + CRX_STATS_SUM_D_EY_MAX] = em;
    }
}

hipError_t crx_launch_race_stats(int which, const crx_stats_kparams& sp, hipStream_t st) {
    const dim3 grid(which == 2 ? (unsigned)sp.n_groups : (unsigned)((sp.batch + 255) / 256)), block(256);
    if (grid.x == 0) return hipSuccess;
    switch (which) {
        case 0: hipLaunchKernelGGL(crx_race_stats_reset_kernel, grid, block, 0, st, sp); break;
        case 1: hipLaunchKernelGGL(crx_race_stats_kernel, grid, block, 0, st, sp); break;
        default: hipLaunchKernelGGL(crx_race_stats_summary_kernel, grid, block, 0, st, sp); break;
    }
    return hipGetLastError();
}

hipError_t crx_launch_race_stats_laps(const crx_stats_kparams_laps& sp, hipStream_t st) {
    if (sp.batch == 0) return hipSuccess;
    hipLaunchKernelGGL(crx_race_stats_laps_kernel, dim3((unsigned)((sp.batch + 255) / 256)), dim3(256), 0, st, sp);
    return hipGetLastError();
}

hipError_t crx_launch_seed(int which, const crx_seed_kparams& sp, hipStream_t st) {
    if (sp.batch == 0) return hipSuccess;
    const dim3 grid((unsigned)((sp.batch + 255) / 256)), block(256);
    if (which == 0) hipLaunchKernelGGL(crx_seed_commit_kernel, grid, block, 0, st, sp);
    else hipLaunchKernelGGL(crx_seed_log_kernel, grid, block, 0, st, sp);
    return hipGetLastError();
}

hipError_t crx_launch_mixed_commit(const crx_mixed_commit_kparams& cp, hipStream_t st) {
    if (cp.batch == 0) return hipSuccess;
    hipLaunchKernelGGL(crx_mixed_commit_kernel, dim3((unsigned)((cp.batch + 255) / 256)), dim3(256), 0, st, cp);
    return hipGetLastError();
}

hipError_t crx_launch_game(int which, const crx_game_kparams& gp, hipStream_t st) {
    if (gp.batch == 0) return hipSuccess;
    const long long n = which == 0 ? (long long)gp.batch * gp.n_cars : (which == 2 ? (long long)gp.batch * (8 * gp.N + 6) : gp.batch);
    if (n == 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    switch (which) {
        case 0: hipLaunchKernelGGL(crx_game_traffic_kernel, grid, block, 0, st, gp); break;
        case 1: hipLaunchKernelGGL(crx_game_masks_kernel, grid, block, 0, st, gp); break;
        case 2: hipLaunchKernelGGL(crx_game_commit_kernel, grid, block, 0, st, gp); break;
        default: hipLaunchKernelGGL(crx_game_log_kernel, grid, block, 0, st, gp); break;
    }
    return hipGetLastError();
}
