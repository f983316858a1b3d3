// crx_prep.hip -- what turns raw scenarios into the arrays a solver reads (paths into the reference's car_racing/):
//   crx_prep_kernel        planner host prep: Bezier references and per-stage ey bounds of every region of a scenario, written in the layout
//                          crx_solve_kernel<0> reads.  One wavefront per scenario, lanes over (region, sample).  Closed-form arithmetic, HBM-bound
//                          (reads ~ (12 + 3V + 2V(N+1)) doubles, writes (V+1)(6 + 3N + 3) doubles per scenario).  Restates
//                            planning/planner_helper.py:43-135   get_bezier_control_points
//                            planning/planner_helper.py:138-153  get_bezier_curve, sampled at t = j/N (overtake_traj_planner.py:105-111)
//                            planning/overtake_traj_planner.py:277-324  ey bounds with the obstacle windows (quirks Q2, Q5)
//   crx_scene_kernel       the front of OvertakeTrajPlanner: vehicles of interest, the partial ey sort, veh_infos, max_delta_v, the predictions in
//                          sorted order.  planning/planner_helper.py:177-201, :218-266, planning/overtake_traj_planner.py:29-42, :66-92
//   crx_trackprep_kernel   the inputs of control.mpc_multi_agents' NLP from the planner's outputs: per-stage targets, window filter, lap offsets
//                          and packing of the sorted vehicles' predictions.  control/control.py:373-382, :293-309
//   crx_cbfprep_kernel     obstacle arrays of control.mpccbf for scripted cars.  control/control.py:500, :519
//   the field family       a field of driven cars, every car of a race predicted by the zero-input roll-out of racing/offboard.py:51-94; the block
//                          shape, the table load, the ego pass of the NLP family and the block-strided gather stand once, ahead of the three:
//     crx_field_prep_kernel     every car the ego of its own NLP.  control/control.py:499-540 (realtime_flag == True)
//     crx_field_traffic_kernel  the racing game's traffic arrays: per ego the other cars of its race as crx_scene_kernel takes them.
//                               planning/overtake_traj_planner.py:77-85
//     crx_mixed_prep_kernel     every car under its own controller: the NLP family for the MPC-CBF cars, the iLQR family's arrays for the iLQR
//                               cars (control/control.py:99-104), and the masks of both launches
//     crx_field_prep_tracks_kernel, crx_mixed_prep_tracks_kernel   the two with race r on track race_track[r] of a track set; the mixed kernel's
//                               text is crx_mixed_prep.h, included once per track source
// The comment in front of each kernel has the rest.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "crx_kparams.h"
#include "crx_wave.h"
#include "crx_num.h"

__global__ void __launch_bounds__(WAVE) crx_prep_kernel(const crx_prep_kparams pp) {
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= pp.n_scen) return;
    const int N = pp.N, V = pp.V, R = V + 1;
    const int nv = min(max(pp.n_veh[s], 0), V);   // device-resident counts cannot be validated on the host: clamp
    const double* xw = pp.x_wrapped + (size_t)6 * s;
    const double* vi = pp.veh_info + (size_t)3 * V * s;
    const double L = pp.lap_length, vw = pp.veh_width, tw = pp.track_width;
    // control points in s (:49-85)
    const double s0 = xw[4];
    double s3 = s0 + pp.prediction_factor * pp.max_dv[s] + pp.lookahead, span;
    if (s0 > s3) { span = s3 + L - s0; s3 = s3 + L; } else { span = s3 - s0; }
    const double s1 = span / 3.0 + s0, s2 = 2.0 * span / 3.0 + s0;
    // end point rides the optimal trajectory (:121-134)
    const double s_end = s3 >= L ? s3 - L : s3;
    const double e3 = s_end <= pp.opt_s[0] ? pp.opt_ey[0] : interp1d<INTERP_BISECT>(pp.opt_s, pp.opt_ey, pp.n_opt, s_end);
    const double e0 = xw[5];   // :95 overrides :87-94
    for (int e = lane; e < R * (N + 1); e += WAVE) {
        const int r = e / (N + 1), j = e - r * (N + 1);
        const int rr = r > nv ? nv : r;   // regions beyond this scenario's vehicles repeat the last one (never selected)
        double e12;
        // no vehicle at all (the reference never plans then: get_overtake_flag is false; its code would index an empty
        // list): the single region gets the curve from the ego to the optimal line, and veh_info is not read
        if (nv == 0) e12 = e3;
        else if (rr == 0) e12 = 0.8 * tw - (-vi[3 * rr + 1] - 0.5 * vw) * 0.2;                       // :98-104
        else if (rr == nv) e12 = -0.8 * tw + (vi[3 * (rr - 1) + 1] - 0.5 * vw) * 0.2;           // :106-112
        else e12 = 0.7 * (vi[3 * rr + 1] + 0.5 * vw) + 0.3 * (vi[3 * (rr - 1) + 1] - 0.5 * vw);   // :113-119
        const double t = j * (1.0 / N), u = 1.0 - t;
        const double b0 = pow(u, 3.0), b1 = 3.0 * t * (u * u), b2 = 3.0 * (t * t) * u, b3 = pow(t, 3.0);   // :139-146
        const size_t o = ((size_t)s * R + r) * (N + 1) + j;
        pp.bez_s[o] = s0 * b0 + s1 * b1 + s2 * b2 + s3 * b3;
        pp.bez_ey[o] = e0 * b0 + e12 * b1 + e12 * b2 + e3 * b3;
    }
    // ey bounds (:277-324): both neighbours impose ey >= ey_obs + W + margin inside their s-window (quirk Q2)
    // The window's ends are formed as the reference forms them, os - length - margin and os + length + margin (:297, :300): with the
    // two widths summed first, an ego one ulp outside an end is taken for inside (0.5 + 0.15 rounds up; tests/golden/front_edges.npz).
    const double ub = tw - 0.5 * vw;
    for (int e = lane; e < R * N; e += WAVE) {
        const int r = e / N, k = e - r * N;
        const double s_nom = xw[4] + (k * pp.dt_ref) * xw[0];                                   // :296 (wrapped copy, Q5)
        double lb = -ub;
        for (int side = 0; side < 2; side++) {
            const int v = side == 0 ? r - 1 : r;                                                // sorted[r-1], sorted[r]
            if (v < 0 || v >= nv) continue;
            double os = pp.obs_s[((size_t)s * V + v) * (N + 1) + k];
            os = wrap_above(os, L);                                                             // :291-292
            if (s_nom >= os - pp.veh_length - pp.safety_margin && s_nom <= os + pp.veh_length + pp.safety_margin)
                lb = fmax(lb, pp.obs_ey[((size_t)s * V + v) * (N + 1) + k] + vw + pp.safety_margin);
        }
        pp.ey_lb[((size_t)s * R + r) * N + k] = lb;
    }
    for (int e = lane; e < R * 6; e += WAVE) {
        const int r = e / 6, c = e - 6 * r;
        pp.x0[((size_t)s * R + r) * 6 + c] = pp.x_raw[(size_t)6 * s + c];                      // :266 (raw state, Q5)
    }
    if (lane < R) pp.ey_ub[(size_t)s * R + lane] = ub;
}

// crx_scene_kernel: the front of OvertakeTrajPlanner (get_overtake_flag, the partial ey sort, veh_infos, agent_info.max_delta_v,
// predictions in sorted order), one wavefront per scenario: the decisions are a few dozen scalar operations every lane runs
// alike, the lanes share the copying of the predictions.  Restates planner_helper.py:177-201, :218-266 and
// overtake_traj_planner.py:29-42, :66-92 (quirks Q3, Q4).
__global__ void __launch_bounds__(WAVE) crx_scene_kernel(const crx_scene_kparams sp) {
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= sp.n_scen) return;
    const crx_scene_desc& d = sp.d;
    const int N1 = d.N + 1, VA = d.n_all_max, V = d.n_veh_max;
    const double* ego = sp.ego_xcurv + (size_t)6 * s;
    const double* vx_ = sp.veh_xcurv + (size_t)6 * VA * s;
    const int na = min(max(sp.n_all[s], 0), VA);
    const double L = d.lap_length, s_e = wrap_above(ego[4], L);
    // vehicles of interest, in dict order (get_overtake_flag :29-42 -> check_ego_agent_distance planner_helper.py:218-266)
    int idx[CRX_MAX_VEH], nv = 0, over = 0;
    unsigned long long hits = 0ull;
    int nh = 0;
    for (int v = 0; v < na; v++) {
        const double dv = fabs(ego[0] - vx_[6 * v]);
        const double s_a = wrap_above(vx_[6 * v + 4], L);
        const double ahead = d.safety_factor * d.veh_length + d.prediction_factor * dv, behind = 1.0 * d.veh_length;
        const bool hit = (s_a - s_e <= ahead && s_a >= s_e) || (s_a + L - s_e <= ahead && s_a + L >= s_e) ||
                         (s_e - s_a <= behind && s_a <= s_e) || (s_e + L - s_a <= behind && s_a <= s_e + L);
        if (hit) { hits |= 1ull << v; nh++; }
    }
    // More vehicles of interest than the n_veh_max slots (the reference has no limit): keep the n_veh_max NEAREST along the
    // track (distance on the closed lap, ties to the earlier one), in dict order -- the policy of hostprep.pack_obstacles on the
    // controller side; `overflow` counts the dropped ones.
    if (nh > V) {
        unsigned long long keep = 0ull;
        for (int k = 0; k < V; k++) {
            int best = -1;
            double bd = 0.0;
            for (int v = 0; v < na; v++) {
                if (!((hits >> v) & 1ull) || ((keep >> v) & 1ull)) continue;
                const double g = wrap_above(vx_[6 * v + 4], L) - s_e;
                const double dist = fmin(fabs(g), fmin(fabs(g + L), fabs(g - L)));
                if (best < 0 || dist < bd) { best = v; bd = dist; }
            }
            keep |= 1ull << best;
        }
        over = nh - V;
        hits = keep;
    }
    for (int v = 0; v < na; v++)
        if ((hits >> v) & 1ull) idx[nv++] = v;
    // partial "sort" (:66-76, quirk Q3): a new vehicle goes to the FRONT if its ey >= the current first one's, else to the back
    int ord[CRX_MAX_VEH];
    for (int k = 0; k < nv; k++) {
        const double e = vx_[6 * idx[k] + 5];
        if (k == 0) ord[0] = idx[0];
        else if (e >= vx_[6 * ord[0] + 5]) { for (int q = k; q > 0; q--) ord[q] = ord[q - 1]; ord[0] = idx[k]; }
        else ord[k] = idx[k];          // (e <= first; a NaN would be dropped by the reference, not representable here)
    }
    // agent_info.max_delta_v over the sorted vehicles (planner_helper.py:177-201)
    double mdv = 0.0;
    for (int k = 0; k < nv; k++) mdv = fmax(mdv, fabs(ego[0] - vx_[6 * ord[k]]));
    if (lane == 0) { sp.n_veh[s] = nv; sp.overflow[s] = over; sp.max_dv[s] = mdv; }
    if (lane < V) sp.order[(size_t)V * s + lane] = lane < nv ? ord[lane] : -1;
    // veh_info rows in ITERATION order (:87-92, quirk Q4): (s, max ey over the prediction, min ey)
    if (lane < V) {
        double vi0 = 0.0, mx = 0.0, mn = 0.0;
        if (lane < nv) {
            const double* pe = sp.pred_ey + ((size_t)s * VA + idx[lane]) * N1;
            vi0 = vx_[6 * idx[lane] + 4]; mx = pe[0]; mn = pe[0];
            for (int j = 1; j < N1; j++) { mx = fmax(mx, pe[j]); mn = fmin(mn, pe[j]); }
        }
        double* vi = sp.veh_info + ((size_t)s * V + lane) * 3;
        vi[0] = vi0; vi[1] = mx; vi[2] = mn;
    }
    // predictions of the sorted vehicles
    for (int e = lane; e < V * N1; e += WAVE) {
        const int k = e / N1, j = e - k * N1;
        const size_t src = ((size_t)s * VA + (k < nv ? ord[k] : 0)) * N1 + j;
        sp.obs_s[((size_t)s * V + k) * N1 + j] = k < nv ? sp.pred_s[src] : 0.0;
        sp.obs_ey[((size_t)s * V + k) * N1 + j] = k < nv ? sp.pred_ey[src] : 0.0;
    }
}

// crx_trackprep_kernel: the inputs of control.mpc_multi_agents' NLP from the planner's outputs, one thread per race:
// per-stage targets (control/control.py:373-382: the selected trajectory's ey, linearly interpolated at the clipped nominal s)
// and the window filter / lap offsets / packing of the sorted vehicles' predictions (:293-309).  Arithmetic of
// crx/hostprep.py tracking_targets, cbf_window, pack_obstacles.
__global__ void __launch_bounds__(256) crx_trackprep_kernel(const crx_trackprep_kparams tp) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= tp.batch) return;
    const int N = tp.N, V = tp.V, N1 = N + 1;
    const double* x = tp.x + (size_t)6 * b;
    const double* tr = tp.traj + (size_t)b * N1 * 6;
    const double L = tp.lap_length, vx = x[0], se = x[4];
    // targets: s clipped to the trajectory's range, scipy interp1d(kind="linear") over the trajectory's (s, ey) columns: the scan of
    // interp1d<INTERP_SCAN> (crx_num.h) at stride 6, written out (the table at the end of crx_num.h says why)
    const double s_lo = tr[4], s_hi = tr[(size_t)N * 6 + 4];
    for (int i = 0; i <= N; i++) {
        double s = se + vx * tp.dt_ref * i;
        s = s < s_lo ? s_lo : s;
        s = s >= s_hi ? s_hi : s;
        int hi = 0;
        while (hi < N1 && tr[(size_t)hi * 6 + 4] < s) hi++;
        hi = hi < 1 ? 1 : (hi > N1 - 1 ? N1 - 1 : hi);
        const int lo = hi - 1;
        const double slope = (tr[(size_t)hi * 6 + 5] - tr[(size_t)lo * 6 + 5]) / (tr[(size_t)hi * 6 + 4] - tr[(size_t)lo * 6 + 4]);
        double* xt = tp.xt + ((size_t)b * N1 + i) * 6;
        xt[0] = vx; xt[1] = 0.0; xt[2] = 0.0; xt[3] = 0.0; xt[4] = 0.0;
        xt[5] = slope * (s - tr[(size_t)lo * 6 + 4]) + tr[(size_t)lo * 6 + 5];
    }
    // obstacles: the safety-time window, lap offsets, packing
    const double margin = tp.safety_time * vx;
    double nce;
    const double dist_ego = lap_fold(se, L, nce);
    const int nv = min(max(tp.n_veh[b], 0), V);
    int n = 0;
    for (int v = 0; v < nv; v++) {
        const double* is = tp.obs_s_in + ((size_t)b * V + v) * N1;
        const double* ie = tp.obs_ey_in + ((size_t)b * V + v) * N1;
        double off;
        if (safety_window(dist_ego, nce, is[0], margin, L, off)) {
            double* os = tp.obs_s + ((size_t)b * V + n) * N1;
            double* oe = tp.obs_ey + ((size_t)b * V + n) * N1;
            for (int j = 0; j < N1; j++) { os[j] = is[j]; oe[j] = ie[j]; }
            tp.lap_off[(size_t)b * V + n] = off;
            n++;
        }
    }
    for (int v = n; v < V; v++) {
        double* os = tp.obs_s + ((size_t)b * V + v) * N1;
        double* oe = tp.obs_ey + ((size_t)b * V + v) * N1;
        for (int j = 0; j < N1; j++) { os[j] = 0.0; oe[j] = 0.0; }
        tp.lap_off[(size_t)b * V + v] = 0.0;
    }
    tp.n_obs[b] = n;
}

// ------------------------------------------------------------------------------------------------
// Obstacle arrays of control.mpccbf for scripted cars (see crx_cbf_prep_dev in include/crx.h): one thread
// per race.  int() of the reference truncates toward zero (control.py:500,519).
// ------------------------------------------------------------------------------------------------
// The race's own text, once: L is the launch's lap length (crx_cbfprep_kernel) or the race's own (crx_cbfprep_laps_kernel).
__device__ __forceinline__ void cbfprep_race(const crx_cbfprep_kparams& cp, int b, double L) {
    const int N = cp.N, V = cp.V;
    const double vx = cp.xcurv[6 * (size_t)b], se = cp.xcurv[6 * (size_t)b + 4];
    const double margin = cp.safety_time * vx;
    double nce;
    const double dist_ego = lap_fold(se, L, nce);
    int n = 0;
    for (int v = 0; v < V; v++) {
        const double s0 = cp.car_s0[(size_t)b * V + v], sv = cp.car_v[(size_t)b * V + v], ey = cp.car_ey[(size_t)b * V + v];
        const double s_now = sv * (cp.t + 0 * cp.dt) + s0;
        double off;
        if (safety_window(dist_ego, nce, s_now, margin, L, off)) {
            double* os = cp.obs_s + ((size_t)b * V + n) * (N + 1);
            double* oe = cp.obs_ey + ((size_t)b * V + n) * (N + 1);
            for (int j = 0; j <= N; j++) {
                const double tj = cp.t + j * cp.dt;
                os[j] = sv * tj + s0;
                oe[j] = ey + 0.0 * tj;
            }
            cp.lap_off[(size_t)b * V + n] = off;
            n++;
        }
    }
    for (int v = n; v < V; v++) {
        double* os = cp.obs_s + ((size_t)b * V + v) * (N + 1);
        double* oe = cp.obs_ey + ((size_t)b * V + v) * (N + 1);
        for (int j = 0; j <= N; j++) { os[j] = 0.0; oe[j] = 0.0; }
        cp.lap_off[(size_t)b * V + v] = 0.0;
    }
    cp.n_obs[b] = n;
}
__global__ void __launch_bounds__(256) crx_cbfprep_kernel(const crx_cbfprep_kparams cp) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= cp.batch) return;
    cbfprep_race(cp, b, cp.lap_length);
}
// crx_cbf_prep_laps_dev: race b folded and offset by lap_lengths[b] (the races of a launch on tracks of their own); cp.lap_length is unused
__global__ void __launch_bounds__(256) crx_cbfprep_laps_kernel(const crx_cbfprep_kparams_laps cp) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= cp.batch) return;
    cbfprep_race(cp, b, cp.lap_lengths[b]);
}

// ------------------------------------------------------------------------------------------------
// The FIELD family: crx_field_prep_kernel, crx_field_traffic_kernel, crx_mixed_prep_kernel (and the two `tracks` kernels).  n_races races of C = n_cars driven cars, every
// car an ego and one of the V = C - 1 others of the egos of its race (see "Field races", "Field games", "Mixed fields" in include/crx.h).
// What the three share stands here, once.
//   block shape   one thread per (race, car); a workgroup of 256 threads owns 256 / C WHOLE races, so what a car reads of the others was
//                 written inside its own workgroup and one block barrier separates the two phases.  The threads past the last whole race of a
//                 block, and the races past n_races of the last block, are not `live`: they only take the barriers (field_block, below) --
//                 every thread of a block reaches every __syncthreads(), none returns before the last one.
//   phase 1       zero_input_rollout (crx_num.h) over the track's segment tables in LDS (load_seg_tables): racing/offboard.py:51-94, N + 1
//                 zero-input Euler steps of the curvilinear state along the track's curvature, `while s > L: s -= L` after every step (:90-91)
//                 as wrap_above.  Trig-bound: 2 (N + 1) sin / cos per car.  Every kernel's roll-out columns 0 .. N are the same bits.
//   phase 2       per ego, the other cars of its race in car order (quirk F5).  nlp_ego_pass: the NLP family's arrays and `clear`;
//                 block_gather: wide [V][W] rows per ego copied by the whole block.
// No loop runs on device data: the trip counts come from the descriptor and n_races.
// A car with a non-finite state predicts non-finite rows, passes nobody's window test (every comparison with a NaN is false), keeps nobody
// itself, and never lowers a `clear`; where its rows are only copied (block_gather) they arrive as bits.
// ------------------------------------------------------------------------------------------------
// The track's segment tables as the plant keeps them (crx_plant_step.h), into the caller's LDS arrays.  Holds a barrier: every thread calls it.
__device__ __forceinline__ void load_seg_tables(const double* track, int n_seg, double* seg_lo, double* seg_hi, double* seg_cv) {
    for (int i = threadIdx.x; i < n_seg; i += blockDim.x) {
        seg_lo[i] = track[6 * i + 3];
        seg_hi[i] = track[6 * i + 3] + track[6 * i + 4];
        seg_cv[i] = track[6 * i + 5];
    }
    __syncthreads();
}

struct field_block {
    int n_live, t, c;    // the block's live threads = its cars; this thread, and its car inside its race
    size_t rc0, rc;      // the block's first car and this thread's: problem / scenario rc of the solver launches (race-major, car-minor)
    bool live;
};
__device__ __forceinline__ field_block field_block_of(int C, int n_races) {
    const int per_block = 256 / C, r0 = blockIdx.x * per_block;   // r0: first race of this block, < n_races by the grid's size
    field_block b;
    b.n_live = min(per_block, n_races - r0) * C;
    b.t = threadIdx.x; b.c = b.t % C;
    b.rc0 = (size_t)r0 * C; b.rc = b.rc0 + b.t;
    b.live = b.t < b.n_live;
    return b;
}

// control/control.py:499-540 with realtime_flag == True, for the ego rc = car c of its race: the window test and the lap offset on column 0
// of each other car's prediction (pred_s, pred_ey: rows of `stride` doubles, the first N1 of them copied), kept cars packed to the front in
// car order, the rest zero; (l_e / 2 + l_o / 2, w_e / 2 + w_o / 2) per kept slot (:532-535) when the cars bring their own dimensions; the
// smallest super-ellipse value against the others at the CURRENT states (below 1: contact) into out.clear when it is given.  keep == false:
// an ego that keeps nobody (its policy is not MPC-CBF, quirk M2); `clear` is computed all the same.
__device__ __forceinline__ void nlp_ego_pass(const double* xcurv, const double* car_dims, const double* pred_s, const double* pred_ey, int stride,
                                             double L, double safety_time, double d_l_sum, double d_w_sum, int degree, int N1, int C, int c,
                                             size_t rc, bool keep, const crx_nlp_obs& out) {
    const int V = C - 1;
    const double* xe = xcurv + 6 * rc;
    const double s_e = xe[4], ey_e = xe[5], margin = safety_time * xe[0];
    double nce;
    const double dist_ego = lap_fold(s_e, L, nce);
    // a car's own (length, width); device-resident dimensions cannot be validated on the host: dim_or_default (crx_num.h)
    const double l_e = car_dims ? dim_or_default(car_dims[2 * rc], d_l_sum) : 0.0;
    const double w_e = car_dims ? dim_or_default(car_dims[2 * rc + 1], d_w_sum) : 0.0;
    int n = 0;
    double clr = INFINITY;
    for (int o = 0; o < C; o++) {   // car order, skipping the ego (quirk F5)
        if (o == c) continue;
        const size_t ro = rc - c + o;
        double l_sum = d_l_sum, w_sum = d_w_sum;
        if (car_dims) {
            l_sum = l_e / 2 + dim_or_default(car_dims[2 * ro], d_l_sum) / 2;
            w_sum = w_e / 2 + dim_or_default(car_dims[2 * ro + 1], d_w_sum) / 2;
        }
        if (out.clear) {
            const double* xo = xcurv + 6 * ro;
            double m = fmod(s_e - xo[4] + L / 2, L);   // Python's %: the sign of the divisor
            if (m < 0.0) m += L;
            const double a = (m - L / 2) / l_sum, b = (ey_e - xo[5]) / w_sum;
            double pa = 1.0, pb = 1.0;
            for (int k = 0; k < degree; k++) { pa *= a; pb *= b; }
            const double h = pa + pb;
            clr = h < clr ? h : clr;
        }
        const double* is = pred_s + ro * stride;
        const double* ie = pred_ey + ro * stride;
        double off;
        if (keep && safety_window(dist_ego, nce, is[0], margin, L, off)) {   // column 0: one estimated step ahead (quirk F2)
            double* os = out.obs_s + (rc * V + n) * N1;
            double* oe = out.obs_ey + (rc * V + n) * N1;
            for (int j = 0; j < N1; j++) { os[j] = is[j]; oe[j] = ie[j]; }
            out.lap_off[rc * V + n] = off;
            if (out.obs_dims) { out.obs_dims[(rc * V + n) * 2] = l_sum; out.obs_dims[(rc * V + n) * 2 + 1] = w_sum; }
            n++;
        }
    }
    for (int v = n; v < V; v++) {
        double* os = out.obs_s + (rc * V + v) * N1;
        double* oe = out.obs_ey + (rc * V + v) * N1;
        for (int j = 0; j < N1; j++) { os[j] = 0.0; oe[j] = 0.0; }
        out.lap_off[rc * V + v] = 0.0;
        if (out.obs_dims) { out.obs_dims[(rc * V + v) * 2] = 0.0; out.obs_dims[(rc * V + v) * 2 + 1] = 0.0; }
    }
    out.n_obs[rc] = n;
    if (out.clear) out.clear[rc] = clr;
}

// NA arrays dst[a] [R C][V][W] filled from rows src[a] [R C][stride]: slot v of ego q of the block holds the first W words of the row of car
// slot_car(q, v) of q's race.  HOLES: a negative slot_car is an empty slot, which gets zeros; without HOLES every slot is held and the copy is
// unconditional (the test costs crx_field_traffic_kernel a branch around every load).  The [V][W] rows of one ego are contiguous and
// consecutive threads are consecutive egos, so what a block writes to each array is ONE contiguous range; its live threads stride over that
// range element by element (a wave stores 512 consecutive bytes; its loads are consecutive inside a row) instead of each walking its own
// ego's rows at a stride of V W doubles.  Called by the live threads, after the barrier that publishes the rows.
template <int NA, bool HOLES, typename SlotCar>
__device__ __forceinline__ void block_gather(const field_block& b, int C, int W, int stride, const double* const (&src)[NA], double* const (&dst)[NA],
                                             SlotCar slot_car) {
    const int row = (C - 1) * W;
    for (int e = b.t; e < b.n_live * row; e += b.n_live) {
        const int q = e / row, m = e - q * row, v = m / W, w = m - W * v;
        const int o = slot_car(q, v);
        const bool held = !HOLES || o >= 0;
        const size_t from = (b.rc0 + (q - q % C) + (held ? o : 0)) * stride + w;
        for (int a = 0; a < NA; a++) dst[a][b.rc0 * row + e] = held ? src[a][from] : 0.0;
    }
}

// Obstacle arrays of control.mpccbf for a field (crx_field_prep_dev, quirks F1-F7): the roll-out, then every car the ego of its own NLP.
__global__ void __launch_bounds__(256) crx_field_prep_kernel(const crx_field_kparams fp) {
    __shared__ double seg_lo[CRX_PLANT_MAX_SEG], seg_hi[CRX_PLANT_MAX_SEG], seg_cv[CRX_PLANT_MAX_SEG];
    const crx_field_desc& d = fp.d;
    load_seg_tables(fp.track, d.n_seg, seg_lo, seg_hi, seg_cv);
    const int N1 = d.N + 1;
    const field_block b = field_block_of(d.n_cars, fp.n_races);
    if (b.live)
        zero_input_rollout(fp.xcurv + 6 * b.rc, seg_lo, seg_hi, seg_cv, d.n_seg, d.lap_length, d.dt, N1, fp.pred_s + b.rc * N1, fp.pred_ey + b.rc * N1);
    __syncthreads();   // the predictions of this block's races are in memory; workgroup scope is all phase 2 needs
    if (!b.live) return;
    nlp_ego_pass(fp.xcurv, fp.car_dims, fp.pred_s, fp.pred_ey, N1, d.lap_length, d.safety_time, d.l_sum, d.w_sum, d.degree, N1, d.n_cars, b.c, b.rc,
                 true, fp.nlp);
}

// The racing game's traffic arrays for a field (crx_field_traffic_dev, quirks F1-F3, F6, G1-G3): what crx_game_traffic_kernel makes of
// scripted cars, made of the other DRIVEN cars of the race -- the inputs of crx_scene_kernel for the n_races * C scenarios with n_all_max =
// n_veh_max = V.  Phase 2 is overtake_traj_planner.py:77-85 (the `else` branch: a driven opponent's get_trajectory_nsteps(N + 1)) per ego:
// slot v of ego c is car o = v + (v >= c).  Pure copies; nothing here computes on a non-finite car's rows.
__global__ void __launch_bounds__(256) crx_field_traffic_kernel(const crx_field_traffic_kparams tp) {
    __shared__ double seg_lo[CRX_PLANT_MAX_SEG], seg_hi[CRX_PLANT_MAX_SEG], seg_cv[CRX_PLANT_MAX_SEG];
    const crx_field_desc& d = tp.d;
    load_seg_tables(tp.track, d.n_seg, seg_lo, seg_hi, seg_cv);
    const int C = d.n_cars, N1 = d.N + 1;
    const field_block b = field_block_of(C, tp.n_races);
    if (b.live)
        zero_input_rollout(tp.xcurv + 6 * b.rc, seg_lo, seg_hi, seg_cv, d.n_seg, d.lap_length, d.dt, N1, tp.pred_s_car + b.rc * N1, tp.pred_ey_car + b.rc * N1);
    __syncthreads();   // the predictions of this block's races are in memory; workgroup scope is all phase 2 needs
    if (!b.live) return;
    tp.n_all[b.rc] = C - 1;
    const auto others = [C](int q, int v) { return v + (v >= q % C ? 1 : 0); };
    const double* const x_src[1] = {tp.xcurv};
    double* const x_dst[1] = {tp.veh_xcurv};
    block_gather<1, false>(b, C, 6, 6, x_src, x_dst, others);
    const double* const p_src[2] = {tp.pred_s_car, tp.pred_ey_car};
    double* const p_dst[2] = {tp.pred_s, tp.pred_ey};
    block_gather<2, false>(b, C, N1, N1, p_src, p_dst, others);
}

// ---- one track per RACE (crx_field_prep_tracks_dev, crx_mixed_prep_tracks_dev): a race is on one track and all its cars share it; the races of
// a launch, and of a block, may be on different tracks.  The block stages all n_tracks * seg_stride rows, padding included, at their own index
// (load_seg_tables over the whole set: crx_plant_tracks_kernel's staging, 12 KB at most); a lane scans the rows of its race's track and
// wraps, folds, windows, lap-offsets and `clear`s with that track's lap length.  What lives on the device cannot be validated on the host:
// race_track[r] is COMPARED before any use and never becomes an address -- a race whose id is outside [0, n_tracks) has no track (ok ==
// false): every car of it writes NaN prediction rows, keeps nobody (n_obs = 0, zero slots, lap_off = 0), its `clear` is NaN, and it still
// takes the block's barrier; n_seg[t] is clamped to [0, seg_stride], so the scan stays inside the track's own rows whatever the array holds.
struct race_track {
    bool ok;
    int row0, n_seg;   // the track's first row in the block's tables and its rows
    double L;
};
__device__ __forceinline__ race_track race_track_of(const crx_race_tracks& set, const field_block& b, int C) {
    race_track k = {false, 0, 0, 1.0};   // (a lap length the folds of a race without a track are harmless with)
    if (!b.live) return k;
    const int t = set.race_track[b.rc / C];
    if (t < 0 || t >= set.n_tracks) return k;
    k.ok = true;
    k.row0 = t * set.seg_stride; k.n_seg = min(max(set.n_seg[t], 0), set.seg_stride);
    k.L = set.lap_length[t];
    return k;
}
__device__ __forceinline__ void nan_rows(int n, double* ps, double* pe) {
    for (int j = 0; j < n; j++) { ps[j] = NAN; pe[j] = NAN; }
}

// crx_field_prep_kernel with race r on track race_track[r]: the same two phases, the same pieces.
__global__ void __launch_bounds__(256) crx_field_prep_tracks_kernel(const crx_field_kparams_tracks fp) {
    __shared__ double seg_lo[CRX_MAX_TRACKS * CRX_PLANT_MAX_SEG], seg_hi[CRX_MAX_TRACKS * CRX_PLANT_MAX_SEG], seg_cv[CRX_MAX_TRACKS * CRX_PLANT_MAX_SEG];
    const crx_field_desc& d = fp.d;
    load_seg_tables(fp.track, fp.set.n_tracks * fp.set.seg_stride, seg_lo, seg_hi, seg_cv);
    const int N1 = d.N + 1;
    const field_block b = field_block_of(d.n_cars, fp.n_races);
    const race_track k = race_track_of(fp.set, b, d.n_cars);
    if (b.live) {
        if (!k.ok) nan_rows(N1, fp.pred_s + b.rc * N1, fp.pred_ey + b.rc * N1);
        else
            zero_input_rollout(fp.xcurv + 6 * b.rc, seg_lo + k.row0, seg_hi + k.row0, seg_cv + k.row0, k.n_seg, k.L, d.dt, N1, fp.pred_s + b.rc * N1,
                               fp.pred_ey + b.rc * N1);
    }
    __syncthreads();   // the predictions of this block's races are in memory; workgroup scope is all phase 2 needs
    if (!b.live) return;
    nlp_ego_pass(fp.xcurv, fp.car_dims, fp.pred_s, fp.pred_ey, N1, k.L, d.safety_time, d.l_sum, d.w_sum, d.degree, N1, d.n_cars, b.c, b.rc, k.ok,
                 fp.nlp);
    if (!k.ok && fp.nlp.clear) fp.nlp.clear[b.rc] = NAN;
}

// crx_mixed_prep_kernel and crx_mixed_prep_tracks_kernel: the kernel's text is crx_mixed_prep.h, included once per track source.
#define CRX_MIXED_KERNEL crx_mixed_prep_kernel
#define CRX_MIXED_KPARAMS crx_mixed_kparams
#define CRX_MIXED_TABLES(mp)                                                                              \
    __shared__ double seg_lo[CRX_PLANT_MAX_SEG], seg_hi[CRX_PLANT_MAX_SEG], seg_cv[CRX_PLANT_MAX_SEG];    \
    __shared__ signed char il_src[256 * CRX_MAX_OBS];   /* [ego of the block][slot]: the car of the ego's race in that slot, -1: empty */ \
    const crx_mixed_desc& d = mp.d;                                                                       \
    load_seg_tables(mp.track, d.n_seg, seg_lo, seg_hi, seg_cv);
#define CRX_MIXED_READ_TRACK(mp, b)
#define CRX_MIXED_LAP d.lap_length
#define CRX_MIXED_SEG(a) a
#define CRX_MIXED_NSEG d.n_seg
#define CRX_MIXED_UNLESS_NO_TRACK(mp, rc, n)
#define CRX_MIXED_POLICY(mp, rc) mp.policy[rc]
#define CRX_MIXED_NO_TRACK_CLEAR(mp, rc)
#include "crx_mixed_prep.h"
#undef CRX_MIXED_KERNEL
#undef CRX_MIXED_KPARAMS
#undef CRX_MIXED_TABLES
#undef CRX_MIXED_READ_TRACK
#undef CRX_MIXED_LAP
#undef CRX_MIXED_SEG
#undef CRX_MIXED_NSEG
#undef CRX_MIXED_UNLESS_NO_TRACK
#undef CRX_MIXED_POLICY
#undef CRX_MIXED_NO_TRACK_CLEAR

// A race without a track (race_track_of): its egos' policy reads as NONE, so m_nlp = m_ilqr = 0, il_n_obs = 0 and every iLQR slot is a hole --
// no solver runs for it.
#define CRX_MIXED_KERNEL crx_mixed_prep_tracks_kernel
#define CRX_MIXED_KPARAMS crx_mixed_kparams_tracks
#define CRX_MIXED_TABLES(mp)                                                                                                                      \
    __shared__ double seg_lo[CRX_MAX_TRACKS * CRX_PLANT_MAX_SEG], seg_hi[CRX_MAX_TRACKS * CRX_PLANT_MAX_SEG], seg_cv[CRX_MAX_TRACKS * CRX_PLANT_MAX_SEG]; \
    __shared__ signed char il_src[256 * CRX_MAX_OBS];                                                                                             \
    const crx_mixed_desc& d = mp.d;                                                                                                               \
    load_seg_tables(mp.track, mp.set.n_tracks * mp.set.seg_stride, seg_lo, seg_hi, seg_cv);
#define CRX_MIXED_READ_TRACK(mp, b) const race_track k = race_track_of(mp.set, b, C);
#define CRX_MIXED_LAP k.L
#define CRX_MIXED_SEG(a) a + k.row0
#define CRX_MIXED_NSEG k.n_seg
#define CRX_MIXED_UNLESS_NO_TRACK(mp, rc, n) if (!k.ok) nan_rows(n, mp.pred_s + rc * n, mp.pred_ey + rc * n); else
#define CRX_MIXED_POLICY(mp, rc) (k.ok ? mp.policy[rc] : CRX_POLICY_NONE)
#define CRX_MIXED_NO_TRACK_CLEAR(mp, rc) if (!k.ok && mp.nlp.clear) mp.nlp.clear[rc] = NAN;
#include "crx_mixed_prep.h"
#undef CRX_MIXED_KERNEL
#undef CRX_MIXED_KPARAMS
#undef CRX_MIXED_TABLES
#undef CRX_MIXED_READ_TRACK
#undef CRX_MIXED_LAP
#undef CRX_MIXED_SEG
#undef CRX_MIXED_NSEG
#undef CRX_MIXED_UNLESS_NO_TRACK
#undef CRX_MIXED_POLICY
#undef CRX_MIXED_NO_TRACK_CLEAR

hipError_t crx_launch_prep(const crx_prep_kparams& pp, hipStream_t st) { return crx_launch_1d(crx_prep_kernel, pp.n_scen, 1, WAVE, st, pp); }
hipError_t crx_launch_scene(const crx_scene_kparams& sp, hipStream_t st) { return crx_launch_1d(crx_scene_kernel, sp.n_scen, 1, WAVE, st, sp); }
hipError_t crx_launch_trackprep(const crx_trackprep_kparams& tp, hipStream_t st) {
    return crx_launch_1d(crx_trackprep_kernel, tp.batch, 256, 256, st, tp);
}
hipError_t crx_launch_cbfprep(const crx_cbfprep_kparams& cp, hipStream_t st) { return crx_launch_1d(crx_cbfprep_kernel, cp.batch, 256, 256, st, cp); }
hipError_t crx_launch_cbfprep_laps(const crx_cbfprep_kparams_laps& cp, hipStream_t st) {
    return crx_launch_1d(crx_cbfprep_laps_kernel, cp.batch, 256, 256, st, cp);
}
// whole races per block: 256 / n_cars of them (n_cars in 1 .. CRX_MAX_OBS + 1, checked by the caller)
hipError_t crx_launch_field_prep(const crx_field_kparams& fp, hipStream_t st) {
    return crx_launch_1d(crx_field_prep_kernel, fp.n_races, 256 / fp.d.n_cars, 256, st, fp);
}
// the same shape (n_cars in 1 .. CRX_MAX_VEH + 1, checked by the caller)
hipError_t crx_launch_field_traffic(const crx_field_traffic_kparams& tp, hipStream_t st) {
    return crx_launch_1d(crx_field_traffic_kernel, tp.n_races, 256 / tp.d.n_cars, 256, st, tp);
}
// the same shape (n_cars in 1 .. CRX_MAX_OBS + 1, checked by the caller)
hipError_t crx_launch_mixed_prep(const crx_mixed_kparams& mp, hipStream_t st) {
    return crx_launch_1d(crx_mixed_prep_kernel, mp.n_races, 256 / mp.d.n_cars, 256, st, mp);
}
// the same shapes with one track per race (n_tracks, seg_stride inside the LDS tables' bounds, checked by the caller)
hipError_t crx_launch_field_prep_tracks(const crx_field_kparams_tracks& fp, hipStream_t st) {
    return crx_launch_1d(crx_field_prep_tracks_kernel, fp.n_races, 256 / fp.d.n_cars, 256, st, fp);
}
hipError_t crx_launch_mixed_prep_tracks(const crx_mixed_kparams_tracks& mp, hipStream_t st) {
    return crx_launch_1d(crx_mixed_prep_tracks_kernel, mp.n_races, 256 / mp.d.n_cars, 256, st, mp);
}
