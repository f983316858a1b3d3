// crx_ilqr.hip -- batched iLQR of the reference's ego controller (control/control.py:64-195 ilqr, control/ilqr_helper.py:4-55),
// one 64-lane wave per problem, FP64, gfx950 only.
//
// One problem: LTI x_{k+1} = A x_k + B u_k, tracking cost (x - xt)' Q (x - xt) + u' R u, exponential repelling term around
// n_obs obstacle predictions (s, ey)[N+1].  The reference's iteration, quirks included (include/crx.h lists them as I1..I6):
//   roll out from u = 0 (I6) -> stage derivatives 0..N-1 (I2, I5) -> backward pass with the eigenvalue-clamped, lambda-regularised
//   Quu (I4) -> full-step forward pass with feedback -> accept iff the barrier-free cost (I3) decreased: lambda /= 10, stop when the
//   relative decrease is below eps; else lambda *= 10, stop when lambda > lamb_max; at most max_iter backward passes.
//
// Lane layout inside the wave:
//   - derivative phase and stage costs: lane k = stage k (N <= 64 = one pass);
//   - backward pass: 36 lanes hold a 6x6 product entry each, 12 lanes the 2x6 ones, the 2x2 eigen-decomposition is closed form and
//     computed redundantly by every lane (wave-uniform);
//   - rollout / forward pass: lanes 0..5 own one state row each and recompute the two inputs of the stage redundantly (identical bits).
// The reference's rollout at the top of an iteration (:106-115) recomputes the trajectory of the last accepted forward pass with the
// same expression and the same operands, so it reproduces that pass's trajectory and cost bit for bit; the kernel therefore rolls out
// once (u = 0) and carries the accepted forward pass's (x, u, cost) over instead of recomputing them.
// The cost sums run sequentially on lane 0 in the reference's order ((cost + l_state) + l_ctrl, stage by stage), so the accept and stop
// tests see the reference's rounding of the sum, not a tree reduction's.
// A, B, Q, R are uniform over the batch: the kernel argument block holds them (scalar loads), LDS a copy for lane-indexed reads.
// Per-problem models (crx_ilqr_solve_models): crx_ilqr_models_kernel is the same body with the two LDS copies of A and B read from
// model_A[b], model_B[b]; every later read goes through LDS.  The shared-model kernel is instantiated without that branch.
#include <hip/hip_runtime.h>
#include <math.h>

#if !defined(__HIP_DEVICE_COMPILE__) || defined(__gfx950__)
#else
#error "crx_ilqr.hip targets gfx950 (MI355X) only"
#endif

#include "crx_kparams.h"
#include "crx_wave.h"

namespace {

// LDS slice of one problem, in doubles (N = horizon)
struct IL {
    int A, B, Q, R, Vx, Vxx, M, S, Qx, Qu, Qxx, Qux, Quu, sc, st, x0, x1, u0, u1, kf, Kf, lx, lc, total;
    __device__ __host__ explicit IL(int N) {
        int o = 0;
        A = o; o += 36; B = o; o += 12; Q = o; o += 36; R = o; o += 4;
        Vx = o; o += 6; Vxx = o; o += 36; M = o; o += 36; S = o; o += 12;
        Qx = o; o += 6; Qu = o; o += 2; Qxx = o; o += 36; Qux = o; o += 12; Quu = o; o += 4;
        sc = o; o += 8;                       // wave-uniform scalars handed from lane 0: [0] cost of a forward pass
        st = o; o += 2 * (N + 1);             // per-stage (l_state, l_ctrl)
        x0 = o; o += 6 * (N + 1); x1 = o; o += 6 * (N + 1);   // accepted / trial trajectory (swapped on accept)
        u0 = o; o += 2 * N; u1 = o; o += 2 * N;
        kf = o; o += 2 * N; Kf = o; o += 12 * N;              // k[i][2], K[i][2][6]
        lx = o; o += 6 * N; lc = o; o += 3 * N;               // l_x[i][6]; barrier block of l_xx[i]: (44, 45, 55)
        total = o;
    }
};

// (x_k - xt)' Q (x_k - xt) (lanes k <= N) and u_k' R u_k (k < N), into st[k][2]
__device__ __forceinline__ void stage_costs(double* sm, const IL& L, int N, int xo, int uo, const double* xt, int lane) {
#pragma unroll 1
    for (int k = lane; k <= N; k += WAVE) {   // N = 64: lane 0 also takes the terminal stage
        double d[6];
#pragma unroll
        for (int c = 0; c < 6; c++) d[c] = sm[xo + 6 * k + c] - xt[c];
        double ls = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            double v = 0.0;
#pragma unroll
            for (int r = 0; r < 6; r++) v += d[r] * sm[L.Q + 6 * r + c];
            ls += v * d[c];
        }
        double lu = 0.0;
        if (k < N) {
            const double a = sm[uo + 2 * k], b = sm[uo + 2 * k + 1];
            lu = (a * sm[L.R + 0] + b * sm[L.R + 2]) * a + (a * sm[L.R + 1] + b * sm[L.R + 3]) * b;
        }
        sm[L.st + 2 * k] = ls;
        sm[L.st + 2 * k + 1] = lu;
    }
    SYNC();
    if (lane == 0) {   // the reference's accumulation order (control.py:106-115, :166-175)
        double c = 0.0;
#pragma unroll 1
        for (int k = 0; k < N; k++) c = (c + sm[L.st + 2 * k]) + sm[L.st + 2 * k + 1];
        sm[L.sc] = c + sm[L.st + 2 * N];
    }
    SYNC();
}

template <bool MODELS>
__device__ __forceinline__ void ilqr_body(const crx_ilqr_kparams& kp) {
    extern __shared__ double sm[];
    const int b = blockIdx.x;
    if (b >= kp.batch) return;
    const int lane = threadIdx.x;
    if (kp.active && kp.active[b] == 0) {
        if (lane == 0) kp.status[b] = CRX_SKIPPED;
        return;
    }
    const int N = kp.N;
    const IL L(N);
    if (lane < 36) { sm[L.A + lane] = MODELS ? kp.model_A[(size_t)36 * b + lane] : kp.A[lane]; sm[L.Q + lane] = kp.Q[lane]; }
    if (lane < 12) sm[L.B + lane] = MODELS ? kp.model_B[(size_t)12 * b + lane] : kp.B[lane];
    if (lane < 4) sm[L.R + lane] = kp.R[lane];
    double xt[6];
#pragma unroll
    for (int c = 0; c < 6; c++) xt[c] = kp.xt[6 * b + c];
    const int n_obs = min(max(kp.n_obs[b], 0), kp.n_obs_max);
    const size_t ob = (size_t)b * kp.n_obs_max;
    // (I5) P1 = diag(0, 0, 0, 0, 1 / l_sum^2, 1 / w_sum^2)
    const double p4 = 1.0 / (kp.l_sum * kp.l_sum), p5 = 1.0 / (kp.w_sum * kp.w_sum);
    const double h0 = 1.0 + kp.margin, g1 = kp.q1 * kp.q2, g2 = kp.q1 * (kp.q2 * kp.q2);

    // (I6) roll out from u = 0 (control.py:86-87,106-115)
    int xa = L.x0, xb = L.x1, ua = L.u0, ub = L.u1;
    if (lane < 6) sm[xa + lane] = kp.x0[6 * b + lane];
    for (int i = lane; i < 2 * N; i += WAVE) sm[ua + i] = 0.0;
    SYNC();
#pragma unroll 1
    for (int k = 0; k < N; k++) {
        if (lane < 6) {
            double v = 0.0;
#pragma unroll
            for (int c = 0; c < 6; c++) v += sm[L.A + 6 * lane + c] * sm[xa + 6 * k + c];
            const double w = sm[L.B + 2 * lane] * sm[ua + 2 * k] + sm[L.B + 2 * lane + 1] * sm[ua + 2 * k + 1];
            sm[xa + 6 * (k + 1) + lane] = v + w;
        }
        SYNC();
    }
    stage_costs(sm, L, N, xa, ua, xt, lane);
    double cost = sm[L.sc];

    double lamb = kp.lamb_init;
    int status = CRX_MAX_ITER, it = 0;
#pragma unroll 1
    while (it < kp.max_iter) {
        it++;
        // ---- stage derivatives, stages 0..N-1 (I2), lane = stage (ilqr_helper.py:4-45)
        if (lane < N) {
            const int k = lane;
            double dx[6];
#pragma unroll
            for (int c = 0; c < 6; c++) dx[c] = sm[xa + 6 * k + c] - xt[c];
            double lx[6];
#pragma unroll
            for (int r = 0; r < 6; r++) {
                double v = 0.0;
#pragma unroll
                for (int c = 0; c < 6; c++) v += (2.0 * sm[L.Q + 6 * r + c]) * dx[c];
                lx[r] = v;
            }
            double c44 = 0.0, c45 = 0.0, c55 = 0.0;
            const double s = sm[xa + 6 * k + 4], ey = sm[xa + 6 * k + 5];
#pragma unroll 1
            for (int o = 0; o < n_obs; o++) {
                // (I5) ds = s_k - s_obs,k - (cyc_ego - cyc_obs) L; the host folds the lap term into lap_off
                const double ds = (s - kp.obs_s[(ob + o) * (N + 1) + k]) - kp.lap_off[ob + o];
                const double de = ey - kp.obs_ey[(ob + o) * (N + 1) + k];
                const double h = h0 - ((ds * p4) * ds + (de * p5) * de);
                const double hd4 = (-2.0 * p4) * ds, hd5 = (-2.0 * p5) * de;
                const double e = exp(kp.q2 * h);
                const double gb = g1 * e, hb = g2 * e;
                lx[4] += gb * hd4;
                lx[5] += gb * hd5;
                c44 += hb * (hd4 * hd4);
                c45 += hb * (hd4 * hd5);
                c55 += hb * (hd5 * hd5);
            }
#pragma unroll
            for (int r = 0; r < 6; r++) sm[L.lx + 6 * k + r] = lx[r];
            sm[L.lc + 3 * k] = c44; sm[L.lc + 3 * k + 1] = c45; sm[L.lc + 3 * k + 2] = c55;
        }
        SYNC();
        // (I2) terminal value = stage N-1's running derivatives
        if (lane < 6) sm[L.Vx + lane] = sm[L.lx + 6 * (N - 1) + lane];
        if (lane < 36) {
            const int r = lane / 6, c = lane % 6;
            double v = 2.0 * sm[L.Q + lane];
            if (r >= 4 && c >= 4) v += sm[L.lc + 3 * (N - 1) + (r - 4) + (c - 4)];
            sm[L.Vxx + lane] = v;
        }
        SYNC();
        // ---- backward pass (control.py:140-160)
#pragma unroll 1
        for (int i = N - 1; i >= 0; i--) {
            // (a) M = A' Vxx, S = B' Vxx, Qx = l_x + A' Vx, Qu = l_u + B' Vx
            if (lane < 36) {
                const int r = lane / 6, c = lane % 6;
                double v = 0.0;
#pragma unroll
                for (int m = 0; m < 6; m++) v += sm[L.A + 6 * m + r] * sm[L.Vxx + 6 * m + c];
                sm[L.M + lane] = v;
            } else if (lane < 48) {
                const int a = (lane - 36) / 6, c = (lane - 36) % 6;
                double v = 0.0;
#pragma unroll
                for (int m = 0; m < 6; m++) v += sm[L.B + 2 * m + a] * sm[L.Vxx + 6 * m + c];
                sm[L.S + lane - 36] = v;
            } else if (lane < 54) {
                const int c = lane - 48;
                double v = 0.0;
#pragma unroll
                for (int m = 0; m < 6; m++) v += sm[L.A + 6 * m + c] * sm[L.Vx + m];
                sm[L.Qx + c] = sm[L.lx + 6 * i + c] + v;
            } else if (lane < 56) {
                const int a = lane - 54;
                double v = 0.0;
#pragma unroll
                for (int m = 0; m < 6; m++) v += sm[L.B + 2 * m + a] * sm[L.Vx + m];
                // l_u = 2 R u_i (ilqr_helper.py:30)
                const double lu = (2.0 * sm[L.R + 2 * a]) * sm[ua + 2 * i] + (2.0 * sm[L.R + 2 * a + 1]) * sm[ua + 2 * i + 1];
                sm[L.Qu + a] = lu + v;
            }
            SYNC();
            // (b) Qxx = l_xx + M A, Qux = S A (I4: no l_ux), Quu = l_uu + S B
            if (lane < 36) {
                const int r = lane / 6, c = lane % 6;
                double v = 0.0;
#pragma unroll
                for (int m = 0; m < 6; m++) v += sm[L.M + 6 * r + m] * sm[L.A + 6 * m + c];
                double l = 2.0 * sm[L.Q + lane];
                if (r >= 4 && c >= 4) l += sm[L.lc + 3 * i + (r - 4) + (c - 4)];
                sm[L.Qxx + lane] = l + v;
            } else if (lane < 48) {
                const int a = (lane - 36) / 6, c = (lane - 36) % 6;
                double v = 0.0;
#pragma unroll
                for (int m = 0; m < 6; m++) v += sm[L.S + 6 * a + m] * sm[L.A + 6 * m + c];
                sm[L.Qux + lane - 36] = v;
            } else if (lane < 52) {
                const int a = (lane - 48) / 2, c = (lane - 48) % 2;
                double v = 0.0;
#pragma unroll
                for (int m = 0; m < 6; m++) v += sm[L.S + 6 * a + m] * sm[L.B + 2 * m + c];
                sm[L.Quu + lane - 48] = 2.0 * sm[L.R + lane - 48] + v;
            }
            SYNC();
            // (c) (I4) Quu^-1 = V diag(1 / (max(l, 0) + lamb)) V' in closed form (symmetric 2x2: one unit eigenvector v of the
            // larger eigenvalue, the other is its normal), k = -Quu^-1 Qu, K = -Quu^-1 Qux; Vx, Vxx with the UNREGULARISED Quu
            const double qa = sm[L.Quu + 0], qd = sm[L.Quu + 3], qb = 0.5 * (sm[L.Quu + 1] + sm[L.Quu + 2]);
            const double half = 0.5 * (qa - qd), mid = 0.5 * (qa + qd), rad = sqrt(half * half + qb * qb);
            const double mu1 = fmax(mid + rad, 0.0) + lamb, mu2 = fmax(mid - rad, 0.0) + lamb;
            double v0 = half >= 0.0 ? half + rad : qb, v1 = half >= 0.0 ? qb : rad - half;
            const double nv = sqrt(v0 * v0 + v1 * v1);
            if (nv > 0.0) { v0 /= nv; v1 /= nv; } else { v0 = 1.0; v1 = 0.0; }
            const double i1 = 1.0 / mu1, i2 = 1.0 / mu2;
            const double w00 = v0 * v0 * i1 + v1 * v1 * i2, w01 = v0 * v1 * (i1 - i2), w11 = v1 * v1 * i1 + v0 * v0 * i2;
            if (lane < 36) {
                const int r = lane / 6, c = lane % 6;
                // K[:, r], K[:, c]; (Quu K)[:, c]
                const double kr0 = -(w00 * sm[L.Qux + r] + w01 * sm[L.Qux + 6 + r]);
                const double kr1 = -(w01 * sm[L.Qux + r] + w11 * sm[L.Qux + 6 + r]);
                const double kc0 = -(w00 * sm[L.Qux + c] + w01 * sm[L.Qux + 6 + c]);
                const double kc1 = -(w01 * sm[L.Qux + c] + w11 * sm[L.Qux + 6 + c]);
                const double t0 = kr0 * sm[L.Quu + 0] + kr1 * sm[L.Quu + 2], t1 = kr0 * sm[L.Quu + 1] + kr1 * sm[L.Quu + 3];
                sm[L.Vxx + lane] = sm[L.Qxx + lane] - (t0 * kc0 + t1 * kc1);
            } else if (lane < 42) {
                const int c = lane - 36;
                const double kc0 = -(w00 * sm[L.Qux + c] + w01 * sm[L.Qux + 6 + c]);
                const double kc1 = -(w01 * sm[L.Qux + c] + w11 * sm[L.Qux + 6 + c]);
                const double f0 = -(w00 * sm[L.Qu + 0] + w01 * sm[L.Qu + 1]), f1 = -(w01 * sm[L.Qu + 0] + w11 * sm[L.Qu + 1]);
                const double t0 = kc0 * sm[L.Quu + 0] + kc1 * sm[L.Quu + 2], t1 = kc0 * sm[L.Quu + 1] + kc1 * sm[L.Quu + 3];
                sm[L.Vx + c] = sm[L.Qx + c] - (t0 * f0 + t1 * f1);
            } else if (lane < 54) {
                const int a = (lane - 42) / 6, c = (lane - 42) % 6;
                const double wa0 = a == 0 ? w00 : w01, wa1 = a == 0 ? w01 : w11;
                sm[L.Kf + 12 * i + 6 * a + c] = -(wa0 * sm[L.Qux + c] + wa1 * sm[L.Qux + 6 + c]);
            } else if (lane < 56) {
                const int a = lane - 54;
                const double wa0 = a == 0 ? w00 : w01, wa1 = a == 0 ? w01 : w11;
                sm[L.kf + 2 * i + a] = -(wa0 * sm[L.Qu + 0] + wa1 * sm[L.Qu + 1]);
            }
            SYNC();
        }
        // ---- full-step forward pass with feedback (control.py:162-172): lanes 0..5 own x rows, recompute u_i redundantly
        if (lane < 6) sm[xb + lane] = sm[xa + lane];
        SYNC();
#pragma unroll 1
        for (int i = 0; i < N; i++) {
            if (lane < 6) {
                double un[2];
#pragma unroll
                for (int a = 0; a < 2; a++) {
                    double f = 0.0;
#pragma unroll
                    for (int c = 0; c < 6; c++) f += sm[L.Kf + 12 * i + 6 * a + c] * (sm[xb + 6 * i + c] - sm[xa + 6 * i + c]);
                    un[a] = (sm[ua + 2 * i + a] + sm[L.kf + 2 * i + a]) + f;
                }
                double v = 0.0;
#pragma unroll
                for (int c = 0; c < 6; c++) v += sm[L.A + 6 * lane + c] * sm[xb + 6 * i + c];
                const double w = sm[L.B + 2 * lane] * un[0] + sm[L.B + 2 * lane + 1] * un[1];
                if (lane < 2) sm[ub + 2 * i + lane] = un[lane];
                sm[xb + 6 * (i + 1) + lane] = v + w;
            }
            SYNC();
        }
        stage_costs(sm, L, N, xb, ub, xt, lane);
        const double cost_new = sm[L.sc];
        // ---- accept / lambda (control.py:177-190)
        if (cost_new < cost) {
            const double rel = fabs((cost_new - cost) / cost);
            int t = xa; xa = xb; xb = t;
            t = ua; ua = ub; ub = t;
            lamb = lamb / kp.lamb_factor;
            cost = cost_new;
            if (rel < kp.eps) { status = CRX_CONVERGED; break; }
        } else {
            lamb = lamb * kp.lamb_factor;
            if (lamb > kp.lamb_max) { status = CRX_STALLED; break; }
        }
    }
    // outputs: the accepted trajectory (the reference returns uvar[:, 0] of it, :195)
    double* X = kp.X + (size_t)b * 6 * (N + 1);
    double* U = kp.U + (size_t)b * 2 * N;
    for (int i = lane; i < 6 * (N + 1); i += WAVE) X[i] = sm[xa + i];
    for (int i = lane; i < 2 * N; i += WAVE) U[i] = sm[ua + i];
    if (lane == 0) {
        kp.cost[b] = cost;
        kp.status[b] = status;
        kp.iters[b] = it;
    }
}

}  // namespace

__global__ void __launch_bounds__(WAVE) crx_ilqr_kernel(const crx_ilqr_kparams kp) { ilqr_body<false>(kp); }
__global__ void __launch_bounds__(WAVE) crx_ilqr_models_kernel(const crx_ilqr_kparams kp) { ilqr_body<true>(kp); }

size_t crx_ilqr_lds_bytes(int N) { return (size_t)IL(N).total * sizeof(double); }

int crx_ilqr_resident_per_cu(int N) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, crx_ilqr_kernel, WAVE, crx_ilqr_lds_bytes(N)) != hipSuccess) return -1;
    return n;
}

hipError_t crx_launch_ilqr(const crx_ilqr_kparams& kp, hipStream_t st) {
    if (kp.batch == 0) return hipSuccess;
    if (kp.model_A)
        hipLaunchKernelGGL(crx_ilqr_models_kernel, dim3(kp.batch), dim3(WAVE), crx_ilqr_lds_bytes(kp.N), st, kp);
    else
        hipLaunchKernelGGL(crx_ilqr_kernel, dim3(kp.batch), dim3(WAVE), crx_ilqr_lds_bytes(kp.N), st, kp);
    return hipGetLastError();
}
