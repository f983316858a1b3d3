// crx_mixed_prep.h -- the mixed field's prep kernel's text, included by crx_prep.hip once per instantiation (no include guard), after the field
// family's shared pieces (load_seg_tables, field_block_of, nlp_ego_pass, block_gather, race_track_of).  The includer defines
//   CRX_MIXED_KERNEL, CRX_MIXED_KPARAMS   the kernel's name and its parameter struct (crx_mixed_kparams or derived from it)
//   CRX_MIXED_TABLES(mp)                  the LDS arrays seg_lo, seg_hi, seg_cv and il_src, `d`, the block's staging call with its barrier
//   CRX_MIXED_READ_TRACK(mp, b)           statements after field_block_of that bring the lane's track (first row, rows, lap length) into registers
//   CRX_MIXED_LAP                         the lap length of the roll-out, the NLP family's fold and window, `clear` and the iLQR lap offset
//   CRX_MIXED_SEG(a), CRX_MIXED_NSEG      the lane's rows of table a, which the roll-out scans, and their number
//   CRX_MIXED_UNLESS_NO_TRACK(mp, rc, n)  in front of the roll-out: nothing, or `if (the race has no track) { n NaN columns } else`
//   CRX_MIXED_POLICY(mp, rc)              the ego's policy code
//   CRX_MIXED_NO_TRACK_CLEAR(mp, rc)      after nlp_ego_pass: nothing, or `clear` = NaN for a race that has no track
// A text include and not a function over the track source, for crx_plant_step.h's reason: crx_mixed_prep_kernel stays what it is, bit for bit --
// the macros of the one-track kernel expand to the tokens that stood in crx_prep.hip before there were any.
//
// The solver inputs of a mixed field (crx_mixed_prep_dev, quirks F1-F3, F6, M1, M2): every car of a race under its own policy, so one launch
// prepares the NLP family for the MPC-CBF cars, the iLQR family's arrays for the iLQR cars (control/control.py:99-104), and the two masks the
// solver launches run under.
//   phase 1  the roll-out runs max(N, N_ilqr) + 1 steps.  Before the barrier each ego also decides, from the INPUTS alone (policies,
//            finiteness of the states), which cars its iLQR slots hold, and leaves that in LDS (il_src: a car index, or -1) -- so the one
//            barrier that publishes the roll-outs publishes the slot map too.
//   phase 2  per ego: nlp_ego_pass (an ego that is not MPCCBF keeps nobody); the iLQR family's lap offsets and counts; then the wide iLQR
//            rows by block_gather, each slot's source looked up in il_src.
// Policy codes are compared, never used as an index.
__global__ void __launch_bounds__(256) CRX_MIXED_KERNEL(const CRX_MIXED_KPARAMS mp) {
    CRX_MIXED_TABLES(mp)
    const int C = d.n_cars, V = C - 1, N1 = d.N + 1, NI1 = d.N_ilqr + 1, NP1 = max(d.N, d.N_ilqr) + 1;
    const field_block b = field_block_of(C, mp.n_races);
    const int t = b.t, c = b.c;
    const size_t rc = b.rc;
    const bool ilqr_on = d.N_ilqr > 0;
    CRX_MIXED_READ_TRACK(mp, b)
    const double L = CRX_MIXED_LAP;
    int pol = CRX_POLICY_NONE;
    bool fin_e = true;
    if (b.live) {
        CRX_MIXED_UNLESS_NO_TRACK(mp, rc, NP1)
        zero_input_rollout(mp.xcurv + 6 * rc, CRX_MIXED_SEG(seg_lo), CRX_MIXED_SEG(seg_hi), CRX_MIXED_SEG(seg_cv), CRX_MIXED_NSEG, L, d.dt, NP1, mp.pred_s + rc * NP1, mp.pred_ey + rc * NP1);
        pol = CRX_MIXED_POLICY(mp, rc);
        for (int k = 0; k < 6; k++) fin_e = fin_e && isfinite(mp.xcurv[6 * rc + k]);
        if (ilqr_on) {   // the slot map of this ego: the finite other cars in car order (all of them, or the last one alone: quirk I1)
            const bool il_e = pol == CRX_POLICY_ILQR && fin_e;
            const int o_last = c == C - 1 ? C - 2 : C - 1;
            int n = 0;
            for (int o = 0; o < C; o++) {
                if (o == c) continue;
                bool fin_o = true;
                for (int k = 0; k < 6; k++) fin_o = fin_o && isfinite(mp.xcurv[6 * (rc - c + o) + k]);
                if (il_e && fin_o && (d.ilqr_obstacles != 0 || o == o_last)) il_src[t * V + n++] = (signed char)o;
            }
            for (int v = n; v < V; v++) il_src[t * V + v] = -1;
        }
    }
    __syncthreads();   // the predictions and the slot maps of this block's races are written; workgroup scope is all phase 2 needs
    if (!b.live) return;
    const bool cbf = pol == CRX_POLICY_MPCCBF;
    nlp_ego_pass(mp.xcurv, mp.car_dims, mp.pred_s, mp.pred_ey, NP1, L, d.safety_time, d.l_sum, d.w_sum, d.degree, N1, C, c, rc, cbf, mp.nlp);
    CRX_MIXED_NO_TRACK_CLEAR(mp, rc)
    mp.m_nlp[rc] = (pol == CRX_POLICY_MPC_LTI || cbf) ? 1 : 0;
    if (!ilqr_on) return;
    // the iLQR family: lap offsets (quirk I5: the obstacle's cycle from column 0 of its roll-out) and the count, from this ego's slot map
    const double s_e = mp.xcurv[6 * rc + 4];
    int ni = 0;
    for (int v = 0; v < V; v++) {
        const int o = il_src[t * V + v];
        double off = 0.0;
        if (o >= 0) { off = (trunc(s_e / L) - trunc(mp.pred_s[(rc - c + o) * NP1] / L)) * L; ni++; }
        mp.il_lap_off[rc * V + v] = off;
    }
    mp.il_n_obs[rc] = ni;
    mp.m_ilqr[rc] = pol == CRX_POLICY_ILQR ? 1 : 0;
    const double* const i_src[2] = {mp.pred_s, mp.pred_ey};
    double* const i_dst[2] = {mp.il_obs_s, mp.il_obs_ey};
    block_gather<2, true>(b, C, NI1, NP1, i_src, i_dst, [&](int q, int v) { return (int)il_src[q * V + v]; });
}
