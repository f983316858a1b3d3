// crx_race_stats_step.h -- the text of the race statistics' sample kernel, included by crx_game.hip once per instantiation (no include guard).
// The includer defines
//   CRX_STATS_KERNEL, CRX_STATS_KPARAMS   the kernel's name and its parameter struct (crx_stats_kparams or derived from it)
//   CRX_STATS_LAP(sp, b)                  car b's lap length: the fold of the gap to every opponent and the half lap of the pass test
//   CRX_STATS_LAP_CHECK(finite, L)        after the state's finiteness test: nothing, or a statement that clears `finite` for a lap length
//                                         that is not positive and finite (device data the host cannot check)
// A text include for crx_plant_step.h's reason: crx_race_stats_kernel stays what it is, bit for bit -- its macros expand to the tokens that
// stood in crx_game.hip before there were any -- and both kernels carry the pragma that makes their bits those of tests/race_stats_model.py.
//
// one sample: the lap counters, then (finite rows only) the track limits, the running sums, and per opponent the super-ellipse value
// of crx_field_prep_kernel's `clear` and the sign change of the lap-folded gap (include/crx.h S2, S3)
__global__ void __launch_bounds__(256) CRX_STATS_KERNEL(const CRX_STATS_KPARAMS sp) {
#pragma clang fp contract(off)   // every operation rounded on its own: tests/race_stats_model.py reproduces the bits in NumPy
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= sp.batch) return;
    const crx_stats_desc& d = sp.d;
    const size_t Bn = (size_t)sp.batch;
    int32_t* si = sp.stat_i + b;
    double* sd = sp.stat_d + b;
    const double* x = sp.xcurv + (size_t)6 * b;
    const double vx = x[0], s_e = x[4], ey_e = x[5], L = CRX_STATS_LAP(sp, b);
    bool finite = true;
    for (int c = 0; c < 6; c++) finite = finite && isfinite(x[c]);
    CRX_STATS_LAP_CHECK(finite, L)
    // line crossings: integers, whatever the state is
    const int lp = sp.laps[b], n_laps = si[CRX_STATS_I_N_LAPS * Bn];
    const long long crossings = (long long)lp - si[CRX_STATS_I_LAPS_PREV * Bn];
    si[CRX_STATS_I_LAPS_PREV * Bn] = lp;
    if (crossings > 0) {
        for (long long k = n_laps; k < n_laps + crossings && k < CRX_STATS_MAX_LAPS; k++) si[(CRX_STATS_I_LAP_STEP + k) * Bn] = sp.sample;
        si[CRX_STATS_I_N_LAPS * Bn] = (int32_t)(n_laps + crossings);
    }
    const int C = d.n_cars, V = C > 0 ? C - 1 : d.n_opp_max;
    if (!finite) {
        if (si[CRX_STATS_I_NONFINITE_STEP * Bn] < 0) si[CRX_STATS_I_NONFINITE_STEP * Bn] = sp.sample;
        for (int j = 0; j < d.n_opp_max; j++) sd[(CRX_STATS_D_DS_PREV + j) * Bn] = NAN;
        return;
    }
    si[CRX_STATS_I_N_SAMPLES * Bn] += 1;
    const double aey = fabs(ey_e);
    if (aey > d.track_width) {
        if (si[CRX_STATS_I_OFF_STEP * Bn] < 0) si[CRX_STATS_I_OFF_STEP * Bn] = sp.sample;
        si[CRX_STATS_I_OFF_SAMPLES * Bn] += 1;
    }
    if (aey > sd[CRX_STATS_D_EY_MAX * Bn]) sd[CRX_STATS_D_EY_MAX * Bn] = aey;
    sd[CRX_STATS_D_SUM_EY2 * Bn] += ey_e * ey_e;
    if (sp.xt) {
        const double dv = vx - sp.xt[(size_t)6 * b];
        sd[CRX_STATS_D_SUM_DV2 * Bn] += dv * dv;
    }
    // field mode: this car's race and its own (length, width), as crx_field_prep_kernel takes them
    const int r = C > 0 ? b / C : 0, c = C > 0 ? b - r * C : -1;
    const double l_e = sp.car_dims ? dim_or_default(sp.car_dims[2 * (size_t)b], d.l_sum) : 0.0;
    const double w_e = sp.car_dims ? dim_or_default(sp.car_dims[2 * (size_t)b + 1], d.w_sum) : 0.0;
    int n = V;
    if (C == 0 && sp.n_opp) { n = sp.n_opp[b]; n = n < 0 ? 0 : (n > V ? V : n); }
    double clr = INFINITY;
    int passes = 0, passed = 0;
    for (int j = 0; j < n; j++) {
        double s_o, ey_o, l_sum = d.l_sum, w_sum = d.w_sum;
        if (C > 0) {                       // the other cars of the race in car order, skipping the ego
            const size_t ro = (size_t)r * C + (j < c ? j : j + 1);
            s_o = sp.xcurv[6 * ro + 4]; ey_o = sp.xcurv[6 * ro + 5];
            if (sp.car_dims) {
                l_sum = l_e / 2 + dim_or_default(sp.car_dims[2 * ro], d.l_sum) / 2;
                w_sum = w_e / 2 + dim_or_default(sp.car_dims[2 * ro + 1], d.w_sum) / 2;
            }
        } else {                           // the scripted cars at their clock
            const size_t io = (size_t)b * V + j;
            s_o = sp.car_v[io] * sp.t + sp.car_s0[io]; ey_o = sp.car_ey[io];
        }
        double* prev = sd + (CRX_STATS_D_DS_PREV + j) * Bn;
        if (!isfinite(s_o) || !isfinite(ey_o)) { *prev = NAN; continue; }
        double m = fmod(s_e - s_o + L / 2, L);   // Python's %: the sign of the divisor
        if (m < 0.0) m += L;
        const double ds = m - L / 2;
        const double a = ds / l_sum, bb = (ey_e - ey_o) / w_sum;
        double pa = 1.0, pb = 1.0;
        for (int k = 0; k < d.degree; k++) { pa *= a; pb *= bb; }
        const double h = pa + pb;
        clr = h < clr ? h : clr;
        const double p = *prev;
        if (isfinite(p) && isfinite(ds)) {
            if (p < 0.0 && ds >= 0.0 && ds - p < L / 2) passes++;
            if (p >= 0.0 && ds < 0.0 && p - ds < L / 2) passed++;
        }
        *prev = ds;
    }
    if (clr < sd[CRX_STATS_D_MIN_CLEAR * Bn]) sd[CRX_STATS_D_MIN_CLEAR * Bn] = clr;
    if (clr < 1.0) {
        if (si[CRX_STATS_I_CONTACT_STEP * Bn] < 0) si[CRX_STATS_I_CONTACT_STEP * Bn] = sp.sample;
        si[CRX_STATS_I_CONTACT_SAMPLES * Bn] += 1;
    }
    if (passes) si[CRX_STATS_I_PASSES * Bn] += passes;
    if (passed) si[CRX_STATS_I_PASSED * Bn] += passed;
    if (sp.flag && sp.flag[b] != 0) si[CRX_STATS_I_FLAG_SAMPLES * Bn] += 1;
}
