// crx_num.h -- small numerics that the prep kernels (crx_prep.hip), the dispatch-order key (crx_order.hip) and the solver's set-up (crx_kernels.hip) share, each stated once.
// Plain per-thread functions over pointers and scalars; not wave primitives (those are crx_wave.h, pinned by tests/wave_model.py).
//
// A site goes through a function here only where the kernel's machine code stayed bit for bit what it was (tools/kernel_diff.py);
// the table at the end lists the others.  One function is here although a caller's code changed: zero_input_rollout(), the roll-out
// crx_field_prep_kernel had written out and crx_field_traffic_kernel needs as well -- same registers, LDS and no scratch, other
// instructions, and crx_field_prep_dev's outputs bit for bit what the parent's library gives.
//
// Floating-point contraction: every including unit includes this header at its head, in the compiler's default state (hipcc: contraction
// on).  interp1d() (slope * dx + y), lap_fold() (s - laps * L) and zero_input_rollout() contain multiply-adds and may fuse, as the written-out
// copies did; none of them is called from under `#pragma clang fp contract(off)` (crx_game_traffic_kernel, crx_lmpcprep.hip;
// crx_race_stats_kernel in crx_game.hip takes dim_or_default() only, which has no arithmetic).
#ifndef CRX_NUM_H
#define CRX_NUM_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>

#include "crx_wave.h"   // wrap_above, wrap_below (zero_input_rollout)

// ---- scipy interp1d(kind="linear") ---------------------------------------------------------------------------------------------
// searchsorted-left (first index with xs[i] >= x), index clipped to [1, n-1], slope form -- so a point outside the table is
// extrapolated from the first / last interval, and x = xs[0] takes the first.  As used at planner_helper.py:121-134,
// overtake_traj_planner.py:332 and control.py:373-382.  Two searches, one clip and slope tail: INTERP_SCAN, a linear scan (tables of
// a horizon's length); INTERP_BISECT, a bisection (the optimal line's few hundred points).  (One function with a compile-time
// search: with the tail as a function of its own under two named searches, crx_prep_kernel's code changes.)
enum InterpSearch { INTERP_SCAN, INTERP_BISECT };
template <InterpSearch HOW>
__device__ __forceinline__ double interp1d(const double* xs, const double* ys, int n, double x) {
    int hi = 0;   // first index with xs[hi] >= x
    if constexpr (HOW == INTERP_BISECT) {
        int end = n;
        while (hi < end) {
            const int mid = (hi + end) >> 1;
            if (xs[mid] < x) hi = mid + 1; else end = mid;
        }
    } else {
        while (hi < n && xs[hi] < x) hi++;
    }
    hi = hi < 1 ? 1 : (hi > n - 1 ? n - 1 : hi);
    const int lo = hi - 1;
    const double slope = (ys[hi] - ys[lo]) / (xs[hi] - xs[lo]);
    return slope * (x - xs[lo]) + ys[lo];
}

// ---- obstacle window of control.mpccbf / mpc_multi_agents (control.py:293-309, :500-519) ----------------------------------------
// lap_fold: a position folded into one lap, and the laps taken off (int() of the reference truncates toward zero).
// safety_window: is an obstacle at s_obs inside +- margin (= safety_time * vx) of the ego, both folded?  lap_off: what brings the
// obstacle's unfolded positions onto the ego's lap.
__device__ __forceinline__ double lap_fold(double s, double L, double& laps) {
    laps = trunc(s / L);
    return s - laps * L;
}
__device__ __forceinline__ bool safety_window(double dist_ego, double laps_ego, double s_obs, double margin, double L, double& lap_off) {
    double laps_obs;
    const double dist_obs = lap_fold(s_obs, L, laps_obs);
    lap_off = (laps_ego - laps_obs) * L;
    return dist_ego > dist_obs - margin && dist_ego < dist_obs + margin;
}

// ---- zero-input roll-out of the reference's driven model (racing/offboard.py:51-94) ----------------------------------------------
// n Euler steps of the curvilinear state x [6] with vx, vy, wz held: every right-hand side on the old state, the curvature at the old s
// folded into one lap -- the first segment with lo <= s <= hi of the n_seg rows seg_lo / seg_hi / seg_cv (the caller's LDS tables, as
// the plant keeps them) -- and `while s > L: s -= L` after every step (:90-91), the roll-out continuing from the wrapped value.
// Writes ps[j], pe[j], j < n: column 0 is one step AHEAD of x.  crx_field_prep_kernel and crx_field_traffic_kernel (crx_prep.hip).
__device__ __forceinline__ void zero_input_rollout(const double* x, const double* seg_lo, const double* seg_hi, const double* seg_cv, int n_seg,
                                                   double L, double dt, int n, double* ps, double* pe) {
    const double vx = x[0], vy = x[1], wz = x[2];
    double epsi = x[3], s = x[4], ey = x[5];
    for (int j = 0; j < n; j++) {
        // curvature at s (wrapped into one lap), first segment with lo <= s <= hi (quirk F6)
        const double sw = wrap_below(wrap_above(s, L), L);
        double curv = 0.0;
        for (int i = 0; i < n_seg; i++)
            if (sw >= seg_lo[i] && sw <= seg_hi[i]) { curv = seg_cv[i]; break; }
        const double ce = cos(epsi), se = sin(epsi);
        const double v_long = (vx * ce - vy * se) / (1 - curv * ey);
        const double epsi_n = epsi + dt * (wz - v_long * curv);
        const double s_n = s + dt * v_long;
        const double ey_n = ey + dt * (vx * se + vy * ce);
        epsi = epsi_n; s = wrap_above(s_n, L); ey = ey_n;   // the roll-out continues from the wrapped value (quirk F3)
        ps[j] = s; pe[j] = ey;
    }
}

// ---- obstacle dimensions ------------------------------------------------------------------------------------------------------
// device-resident dimensions cannot be validated on the host (the host-pointer entry point rejects them): a non-positive or
// non-finite entry falls back to the descriptor's value instead of turning the rows into inf / NaN
__device__ __forceinline__ double dim_or_default(double v, double dflt) { return (!(v > 0.0) || !isfinite(v)) ? dflt : v; }

// ---- Sites that are NOT shared, and why each stays ---------------------------------------------------------------------------------
// "code changes": as in crx_ipm.h -- same arithmetic, but through a function the kernel's machine code is no longer what it was.
// Lines as of this header's last edit; the kernel and its comment "crx_num.h" find the site.
//   strided interp1d        crx_trackprep_kernel (crx_prep.hip:177-189)      the scan over the trajectory's rows (stride 6): code changes through a
//                                                                            strided interp1d, also with the column offsets as template parameters
//   zeroed obstacle slots   crx_trackprep_kernel (crx_prep.hip:209-214)      code changes in crx_trackprep_kernel with any shared form, down to the inner
//                           crx_cbfprep_kernel (crx_prep.hip:247-252)        loop alone; a function with one caller is no sharing, so both copies stay.
//                                                                            (The field family's tail is inside nlp_ego_pass, crx_prep.hip, which its
//                                                                            two kernels share whole; these two kernels must stay bit for bit)
//   super-ellipse value     crx_order_key (crx_order.hip:46-48, :62-64)      code changes as a lambda and as a function (the loop over the degree)
//                           crx_race_stats_kernel (crx_game.hip:289-296)     under `#pragma clang fp contract(off)`, nlp_ego_pass (crx_prep.hip) is
//                                                                            not: l_e / 2 + l_o / 2 can fuse in one and not in the other, so the
//                                                                            pair geometry of the field lives in nlp_ego_pass and here, written out
//   curvature lookup        the plant (crx_plant_step.h: LDS tables), crx_lmpcprep.hip (global table, contraction off): two storage forms; left alone

#endif
