// crx_plant_step.h -- the plant kernel's text, included by crx_plant.hip once per instantiation (no include guard).  The includer defines
//   CRX_PLANT_KERNEL, CRX_PLANT_KPARAMS   the kernel's name and its parameter struct (crx_plant_kparams or derived from it)
//   CRX_PLANT_READ_PARAMS(pk, b)          statements after the bounds check that bring car b's BicycleDynamicsParam values into registers
//   CRX_PLANT_P(name)                     how the sub-step loop names one of m, lf, lr, Iz, Df, Cf, Bf, Dr, Cr, Br
//   CRX_PLANT_TABLES(pk)                  the LDS arrays seg_lo, seg_hi, seg_cv, `d`, the block's staging loop and its barrier
//   CRX_PLANT_READ_TRACK(pk, b)           statements after CRX_PLANT_READ_PARAMS that bring car b's track (rows, first row, lap length) into registers
//   CRX_PLANT_NSEG, CRX_PLANT_ROW(a, i)   the rows the curvature scan runs over and row i of table a among them
//   CRX_PLANT_LAP                         the lap length of the two wraps and of the final `s > L` test
// A text include and not a template over the parameter source (as crx_ilqr.hip's MODELS is): the step inlined into a kernel from a
// __device__ function compiles crx_plant_kernel to other code than the kernel written out (the block-size read of the table loop and
// commuted multiplies in the sub-step loop), and the shipped crx_plant_kernel stays what it is, bit for bit: the
// macros of the one-table kernels expand to the tokens that stood here before there were any.
__global__ void __launch_bounds__(256) CRX_PLANT_KERNEL(const CRX_PLANT_KPARAMS pk) {
    CRX_PLANT_TABLES(pk)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= pk.batch) return;
    CRX_PLANT_READ_PARAMS(pk, b)
    CRX_PLANT_READ_TRACK(pk, b)
    double vx = pk.xcurv[6 * b], vy = pk.xcurv[6 * b + 1], wz = pk.xcurv[6 * b + 2];
    double epsi = pk.xcurv[6 * b + 3], s = pk.xcurv[6 * b + 4], ey = pk.xcurv[6 * b + 5];
    double psi = pk.xglob[6 * b + 3], X = pk.xglob[6 * b + 4], Y = pk.xglob[6 * b + 5];
    const double delta = pk.u[(size_t)pk.u_stride * b], acc = pk.u[(size_t)pk.u_stride * b + 1], dt = d.dt_sub;
    const double sd = sin(delta), cd = cos(delta);
    for (int it = 0; it < d.n_sub; it++) {
        // curvature at s (wrapped into one lap), first segment with lo <= s <= hi
        double sw = s;
        sw = wrap_below(wrap_above(sw, CRX_PLANT_LAP), CRX_PLANT_LAP);
        double curv = 0.0;
        for (int i = 0; i < CRX_PLANT_NSEG; i++)
            if (sw >= CRX_PLANT_ROW(seg_lo, i) && sw <= CRX_PLANT_ROW(seg_hi, i)) { curv = CRX_PLANT_ROW(seg_cv, i); break; }
        // tyre slip angles and lateral forces (the reference uses lf for the rear axle too, :25)
        const double slip_f = delta - atan2(vy + CRX_PLANT_P(lf) * wz, vx);
        const double slip_r = -atan2(vy - CRX_PLANT_P(lf) * wz, vx);
        const double Fyf = 2 * CRX_PLANT_P(Df) * sin(CRX_PLANT_P(Cf) * atan(CRX_PLANT_P(Bf) * slip_f));
        const double Fyr = 2 * CRX_PLANT_P(Dr) * sin(CRX_PLANT_P(Cr) * atan(CRX_PLANT_P(Br) * slip_r));
        const double dvx = acc - 1 / CRX_PLANT_P(m) * Fyf * sd + wz * vy;
        const double dvy = 1 / CRX_PLANT_P(m) * (Fyf * cd + Fyr) - wz * vx;
        const double dwz = 1 / CRX_PLANT_P(Iz) * (CRX_PLANT_P(lf) * Fyf * cd - CRX_PLANT_P(lr) * Fyr);
        const double ce = cos(epsi), se = sin(epsi), cp = cos(psi), sp = sin(psi);
        const double v_long = (vx * ce - vy * se) / (1 - curv * ey);
        const double psi_n = psi + dt * wz;
        const double X_n = X + dt * (vx * cp - vy * sp), Y_n = Y + dt * (vx * sp + vy * cp);
        const double epsi_n = epsi + dt * (wz - v_long * curv);
        const double s_n = s + dt * v_long;
        const double ey_n = ey + dt * (vx * se + vy * ce);
        const double vx_n = vx + dt * dvx, vy_n = vy + dt * dvy, wz_n = wz + dt * dwz;
        vx = vx_n; vy = vy_n; wz = wz_n; epsi = epsi_n; s = s_n; ey = ey_n; psi = psi_n; X = X_n; Y = Y_n;
    }
    if (pk.wrap && s > CRX_PLANT_LAP) {   // ModelBase.update_memory (base.py:795-819)
        s -= CRX_PLANT_LAP;
        if (pk.laps) pk.laps[b] += 1;
    }
    double* g = pk.xglob_next + 6 * (size_t)b;
    double* c = pk.xcurv_next + 6 * (size_t)b;
    g[0] = vx; g[1] = vy; g[2] = wz; g[3] = psi; g[4] = X; g[5] = Y;
    if (pk.noise_z) {
        // bounded process noise (utils/base.py:929-939): clip(z sigma, +-lim), HALF of it added to the curvilinear velocities
        // only -- the global-frame copy stays clean (the next step reads its velocities from xcurv, vehicle_dynamics.py:17-19)
        const double* z = pk.noise_z + 3 * (size_t)b;
        vx += 0.5 * fmax(-0.05, fmin(z[0] * 0.01, 0.05));
        vy += 0.5 * fmax(-0.1, fmin(z[1] * 0.01, 0.1));
        wz += 0.5 * fmax(-0.05, fmin(z[2] * 0.005, 0.05));
    }
    c[0] = vx; c[1] = vy; c[2] = wz; c[3] = epsi; c[4] = s; c[5] = ey;
}
