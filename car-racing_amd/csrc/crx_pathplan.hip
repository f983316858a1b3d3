// crx_pathplan.hip -- the overtake PATH planner around its QPs (remainder):
//   crx_pathprep_kernel     obstacle rows, Bezier control points and polylines, s samples, the two references, side rows and end points of
//                           every region of a scenario, written in the layout crx_path_kernel reads
//   crx_path_masked_kernel  the path QP (crx_path_qp.h, as crx_path.hip's crx_path_kernel) with a per-QP mask
//   crx_pathselect_kernel   first arg-min of the region costs and the target trajectory with its speed profile
//
// Restates (paths into the reference's car_racing/; quirks P1-P8 are spelled out at crx_pathprep_desc in include/crx.h):
//   planning/overtake_path_planner.py:60-100, :113-143, :173-197 (prep and selection), :199-318 (the QP)
//   planning/planner_helper.py:43-135 get_bezier_control_points, :138-153 get_bezier_curve, :177-201 get_agent_info
// The host mirror (planning/overtake_path_planner.py of this package) is the yardstick: every product and sum of the prep and selection
// kernels is rounded on its own, in the mirror's order -- contraction is off from the pragma below on (AFTER the QP's text, which keeps the
// compiler's default as in crx_path.hip), the shared headers' helpers that may fuse are not used.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "crx_kparams.h"
#include "crx_wave.h"
#include "crx_ipm.h"

#define CRX_PATH_KERNEL crx_path_masked_kernel
#define CRX_PATH_KPARAMS crx_path_kparams_masked
#define CRX_PATH_SKIP(pp, b, lane)                                                                          \
    if (pp.active && pp.active[b] == 0) {                                                                    \
        if (lane == 0) { pp.cost[b] = INFINITY; pp.status[b] = CRX_SKIPPED; pp.iters[b] = 0; }              \
        return;                                                                                              \
    }
#include "crx_path_qp.h"

#pragma clang fp contract(off)

namespace {
// `while (s >= L) s -= L` (:233-234) / `while (s > L) s -= L` (:184-197, planner_helper.py:39-42) with a bounded trip count: four laps by
// the loop, the rest in closed form (the rounded quotient may leave one lap)
template <bool STRICT>
__device__ __forceinline__ double path_wrap(double s, double L) {
    auto over = [L](double v) { return STRICT ? v > L : v >= L; };
#pragma unroll 1
    for (int i = 0; i < 4 && over(s); i++) s = s - L;
    if (over(s) && s < 1e300) {
        s = s - L * (STRICT ? ceil(s / L) - 1.0 : floor(s / L));
        if (over(s)) s = s - L;
    }
    return s;
}

// hostprep.interp_clipped: x clipped into the table, searchsorted-left, index clipped to [1, n-1], slope form
__device__ __forceinline__ double path_interp(const double* xs, const double* ys, int n, double x) {
    x = fmin(fmax(x, xs[0]), xs[n - 1]);
    int hi = 0, end = n;
    while (hi < end) {
        const int mid = (hi + end) >> 1;
        if (xs[mid] < x) hi = mid + 1; else end = mid;
    }
    hi = hi < 1 ? 1 : (hi > n - 1 ? n - 1 : hi);
    const int lo = hi - 1;
    const double slope = (ys[hi] - ys[lo]) / (xs[hi] - xs[lo]);
    return slope * (x - xs[lo]) + ys[lo];
}

// what every lane of crx_pathprep_kernel and the thread of crx_pathselect_kernel decide alike about a scenario
__device__ __forceinline__ int path_n_veh(const crx_pathplan_kparams& pp, int s) { return min(max(pp.n_veh[s], 0), pp.d.n_veh_max); }
__device__ __forceinline__ bool path_skipped(const crx_pathplan_kparams& pp, int s) {
    return path_n_veh(pp, s) == 0 || (pp.active && pp.active[s] == 0);
}
}   // namespace

// One wavefront per scenario, lanes over (region, sample).  The scalar part (P1-P3, a few dozen operations) every lane runs alike; the
// polylines go through LDS because lane (r, j) interpolates in the whole polyline of its region.  HBM: 14 + V (1 + N+1) doubles and the
// table look-ups in, (V+1)(4 (N+1) + 2) + 1 doubles out per scenario.
__global__ void __launch_bounds__(WAVE) crx_pathprep_kernel(const crx_pathplan_kparams pp) {
    __shared__ double ps[CRX_MAX_N + 1], pe[CRX_MAX_REGIONS][CRX_MAX_N + 1];
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= pp.n_scen) return;
    const crx_pathprep_desc& d = pp.d;
    const int N = d.N, N1 = N + 1, V = d.n_veh_max, R = V + 1, VA = d.n_all_max;
    const int nv = path_n_veh(pp, s);
    if (path_skipped(pp, s)) {   // not planned: the prep outputs keep their contents, the QPs of the scenario are masked out
        if (pp.qp_active && lane < R) pp.qp_active[(size_t)s * R + lane] = 0;
        return;
    }
    if (pp.qp_active && lane < R) pp.qp_active[(size_t)s * R + lane] = 1;
    const double* xw = pp.x_wrapped + (size_t)6 * s;
    const double* xr = pp.x_raw + (size_t)6 * s;
    const double L = d.lap_length, tw = d.track_width, vw = d.veh_width, mdv = pp.max_dv[s];
    const double ego_s = xr[4], ego_ey = xr[5];
    // P1: rows (s, max ey, min ey) of the sorted vehicles (:60-75)
    double vs[CRX_MAX_VEH], mx[CRX_MAX_VEH], mn[CRX_MAX_VEH];
    bool fin = isfinite(xw[4]) && isfinite(xw[5]) && isfinite(ego_s) && isfinite(ego_ey) && isfinite(mdv);
#pragma unroll
    for (int k = 0; k < CRX_MAX_VEH; k++) {
        vs[k] = 0.0; mx[k] = 0.0; mn[k] = 0.0;
        if (k < nv) {
            const int v = min(max(pp.order[(size_t)V * s + k], 0), VA - 1);
            vs[k] = pp.veh_xcurv[((size_t)VA * s + v) * 6 + 4];
            const double* oe = pp.obs_ey + ((size_t)s * V + k) * N1;
            mx[k] = oe[0]; mn[k] = oe[0];
            for (int j = 1; j < N1; j++) { mx[k] = fmax(mx[k], oe[j]); mn[k] = fmin(mn[k], oe[j]); }
            // (fmax / fmin drop a NaN: the sum does not)
            double acc = vs[k];
            for (int j = 0; j < N1; j++) acc += oe[j];
            fin = fin && isfinite(acc);
        }
    }
    // P2: control points (planner_helper.py:43-135) from the WRAPPED ego state
    const double s0 = xw[4];
    double s3 = s0 + d.prediction_factor * mdv + d.lookahead, cspan;
    if (s0 > s3) { cspan = s3 + L - s0; s3 = s3 + L; } else { cspan = s3 - s0; }
    const double s1 = cspan / 3.0 + s0, s2 = 2.0 * cspan / 3.0 + s0;
    const double s_end = s3 >= L ? s3 - L : s3;
    const bool above = !(s_end <= pp.opt_s[0]) && s_end > pp.opt_s[d.n_opt - 1];   // the reference raises (interp1d bounds_error)
    const double e3 = s_end <= pp.opt_s[0] ? pp.opt_ey[0] : path_interp(pp.opt_s, pp.opt_ey, d.n_opt, s_end);
    // P3: span (:117-127, :230-240) with max_s of get_agent_info (planner_helper.py:177-201)
    double max_s = -INFINITY;
#pragma unroll
    for (int k = 0; k < CRX_MAX_VEH; k++)
        if (k < nv) max_s = fmax(max_s, vs[k] <= d.next_lap_range ? vs[k] + L : vs[k]);
    max_s = path_wrap<true>(max_s, L);
    const double span = max_s + d.safety_factor * d.veh_length + d.prediction_factor * mdv - ego_s;
    const bool bad = !fin || above || !isfinite(span);
    if (lane == 0) pp.span[s] = bad ? NAN : span;
    if (bad) {   // CRX_OUT_OF_DOMAIN: NaN everywhere, the QPs answer CRX_INFEASIBLE
        for (int e = lane; e < R * N1; e += WAVE) {
            const size_t o = (size_t)s * R * N1 + e;
            pp.opt[o] = NAN; pp.bez[o] = NAN; pp.lb[o] = NAN; pp.ub[o] = NAN;
        }
        if (lane < R) { pp.e0[(size_t)s * R + lane] = NAN; pp.eN[(size_t)s * R + lane] = NAN; }
        return;
    }
    // polylines at t = j (1 / N) (:88-100, planner_helper.py:138-153); the s coordinates are the same for every region
    for (int e = lane; e < R * N1; e += WAVE) {
        const int r = e / N1, j = e - r * N1;
        const int rr = r > nv ? nv : r;   // regions beyond this scenario's vehicles repeat the last one (never selected)
        double e12;
        if (rr == 0) e12 = 0.8 * tw - (-mx[0] - 0.5 * vw) * 0.2;                               // planner_helper.py:98-104
        else if (rr == nv) e12 = -0.8 * tw + (mx[rr - 1] - 0.5 * vw) * 0.2;                    // :106-112
        else e12 = 0.7 * (mx[rr] + 0.5 * vw) + 0.3 * (mx[rr - 1] - 0.5 * vw);                  // :113-119
        const double t = j * (1.0 / N), u = 1.0 - t;
        const double b0 = pow(u, 3.0), b1 = 3.0 * t * (u * u), b2 = 3.0 * (t * t) * u, b3 = pow(t, 3.0);
        if (r == 0) ps[j] = s0 * b0 + s1 * b1 + s2 * b2 + s3 * b3;
        pe[r][j] = xw[5] * b0 + e12 * b1 + e12 * b2 + e3 * b3;
    }
    SYNC();
    const double reach = d.safety_factor * d.veh_length, side = d.safety_factor * vw;
    for (int e = lane; e < R * N1; e += WAVE) {
        const int r = e / N1, j = e - r * N1;
        const int rr = r > nv ? nv : r;
        // P4: the sample position (:232-245)
        double s_tmp = ego_s + span * j / N;
        s_tmp = path_wrap<false>(s_tmp, L);
        if (s_tmp <= pp.opt_s[0]) s_tmp = pp.opt_s[0];
        s_tmp = fmin(fmax(s_tmp, ps[0]), ps[N]);
        const size_t o = ((size_t)s * R + r) * N1 + j;
        pp.opt[o] = path_interp(pp.opt_s, pp.opt_ey, d.n_opt, s_tmp);                          // :248
        pp.bez[o] = path_interp(ps, pe[r], N1, s_tmp);                                         // :250
        // P5: side rows (:266-299) merged with the track box
        double lb = -tw, ub = tw;
        if (rr > 0) {                                                                           // left neighbour: sorted[r-1]
            const double front = path_wrap<true>(vs[rr - 1] + reach, L), rear = path_wrap<true>(vs[rr - 1] - reach, L);
            if (!(s_tmp < rear || s_tmp > front)) {
                const double bound = mn[rr - 1] - side;
                if (!(j == 0 && ego_ey >= bound)) ub = fmin(ub, bound);
            }
        }
        if (rr < nv) {                                                                          // right neighbour: sorted[r]
            const double front = path_wrap<true>(vs[rr] + reach, L), rear = path_wrap<true>(vs[rr] - reach, L);
            if (!(s_tmp < rear || s_tmp > front)) {
                const double bound = mx[rr] + side;
                if (!(j == 0 && ego_ey <= bound)) lb = fmax(lb, bound);
            }
        }
        pp.lb[o] = lb; pp.ub[o] = ub;
    }
    if (lane < R) { pp.e0[(size_t)s * R + lane] = ego_ey; pp.eN[(size_t)s * R + lane] = e3; }   // P6
}

// One thread per scenario: P7 (first arg-min, :313-317) and P8 (target with its speed profile, :113-143, :173-182).
__global__ void __launch_bounds__(256) crx_pathselect_kernel(const crx_pathplan_kparams pp) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= pp.n_scen) return;
    const crx_pathprep_desc& d = pp.d;
    const int N = d.N, N1 = N + 1, R = d.n_veh_max + 1;
    if (path_skipped(pp, s)) {   // target untouched
        pp.flag[s] = -1; pp.plan_status[s] = CRX_SKIPPED;
        return;
    }
    const int nv = path_n_veh(pp, s);
    const double* xw = pp.x_wrapped + (size_t)6 * s;
    const double ego_s = pp.x_raw[(size_t)6 * s + 4], span = pp.span[s], L = d.lap_length;
    double* tg = pp.target + (size_t)s * N1 * 6;
    bool ok = isfinite(span);   // (NaN: crx_pathprep_kernel found the scenario out of domain)
    for (int c = 0; c < 6; c++) ok = ok && isfinite(xw[c]);
    double s_q = 0.0;
    const double s_end = ego_s + span * N / N;
    if (ok) {
        if (s_end >= L) s_q = s_end - L < pp.opt_s[0] ? pp.opt_s[0] : s_end - L;              // :129-137
        else if (s_end < pp.opt_s[0]) s_q = pp.opt_s[0];
        else s_q = s_end;
        ok = !(s_q > pp.opt_s[d.n_opt - 1]);                                                  // the reference raises
    }
    if (!ok) {
        for (int e = 0; e < 6 * N1; e++) tg[e] = NAN;
        pp.flag[s] = -1; pp.plan_status[s] = CRX_OUT_OF_DOMAIN;
        return;
    }
    int flag = 0;
    double best = INFINITY;
    for (int r = 0; r <= nv; r++) {
        const double c = pp.cost[(size_t)s * R + r];
        if (c < best) { best = c; flag = r; }
    }
    const double* E = pp.E + ((size_t)s * R + flag) * N1;
    const double vx_t = path_interp(pp.opt_s, pp.opt_vx, d.n_opt, s_q);
    const double delta_t = 2.0 * (s_end - xw[4]) / (vx_t + xw[0]);
    double a = (vx_t - xw[0]) / delta_t;
    a = a < -d.a_max_plan ? -d.a_max_plan : (a > d.a_max_plan ? d.a_max_plan : a);             // np.clip: a NaN stays
    for (int j = 0; j < N1; j++) {
        double* row = tg + 6 * j;
        const double sj = j == 0 ? xw[4] : ego_s + span * j / N;                               // row 0 was overwritten before the speeds
        row[0] = j < N ? sqrt(xw[0] * xw[0] + 2.0 * a * (sj - xw[4])) : 0.0;
        row[1] = j == 0 ? xw[1] : 0.0; row[2] = j == 0 ? xw[2] : 0.0; row[3] = j == 0 ? xw[3] : 0.0;
        row[4] = sj;
        row[5] = j == 0 ? xw[5] : E[j];
    }
    pp.flag[s] = flag; pp.plan_status[s] = CRX_CONVERGED;
}

hipError_t crx_launch_path_masked(const crx_path_kparams_masked& pp, hipStream_t st) {
    return crx_launch_1d(crx_path_masked_kernel, pp.batch, 1, WAVE, st, pp);
}
hipError_t crx_launch_pathprep(const crx_pathplan_kparams& pp, hipStream_t st) { return crx_launch_1d(crx_pathprep_kernel, pp.n_scen, 1, WAVE, st, pp); }
hipError_t crx_launch_pathselect(const crx_pathplan_kparams& pp, hipStream_t st) {
    return crx_launch_1d(crx_pathselect_kernel, pp.n_scen, 256, 256, st, pp);
}
