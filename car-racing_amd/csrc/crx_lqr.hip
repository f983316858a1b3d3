// crx_lqr.hip -- batched design of the reference's LQR tracking controller (control/control.py:28-61 lqr) and its control law,
// FP64, gfx950 only.
//
// crx_lqr_design_kernel: one 64-lane wave per model (A, B), the reference's Riccati fixed point with its quirks (include/crx.h
// lists them as L1..L4), in the operation order of the host mirror control._lqr_gain:
//   PB = P B;  P' = ((A' P) A - ((((A' PB) inv(R + B' PB)) B') P) A) + Q;  K = ((inv((B' P) B + R) B') P) A
// Lane layout: 36 lanes hold one entry of a 6x6 product each, 12 lanes one of a 6x2 / 2x6 product, 4 lanes the 2x2 ones; the 2x2
// inverse is the plain adjugate over the determinant, computed redundantly by every lane (wave-uniform).  Every product is an
// LDS round trip behind SYNC(); every sum runs in ascending index order.  The stop test max|P' - P| < eps is a wave ballot of
// !(|P' - P| < eps) over the 36 entry lanes -- the same decision as the maximum, without a reduction.  One wave, one workgroup,
// one model: a design does not depend on the batch or on the model's position in it.
// crx_lqr_step_kernel: u = -K (x - xt), one thread per car.
#include <hip/hip_runtime.h>
#include <math.h>

#if !defined(__HIP_DEVICE_COMPILE__) || defined(__gfx950__)
#else
#error "crx_lqr.hip targets gfx950 (MI355X) only"
#endif

#include "crx_kparams.h"
#include "crx_wave.h"

namespace {

// LDS slice of one model, in doubles
enum : int {
    L_A = 0, L_B = L_A + 36, L_Q = L_B + 12, L_R = L_Q + 36, L_P = L_R + 4,
    L_T = L_P + 36,    // 6x6 scratch: A' P, then (W B') P
    L_V = L_T + 36,    // 6x6 scratch: W B'
    L_PB = L_V + 36,   // 6x2: P B; the gain phase keeps B' P (2x6) here
    L_S = L_PB + 12,   // 6x2: A' PB, then W = (A' PB) inv(G); the gain phase keeps inv(G) B' and (inv(G) B') P (2x6) here
    L_S2 = L_S + 12,
    L_G = L_S2 + 12,   // 2x2
    L_TOTAL = L_G + 4
};

// plain 2x2 inverse of g (row-major), wave-uniform; false: zero or non-finite determinant (L4)
__device__ __forceinline__ bool inv2(const double* g, double* w) {
    const double a = g[0], b = g[1], c = g[2], d = g[3];
    const double det = a * d - b * c;
    if (!(fabs(det) > 0.0) || !(fabs(det) < INFINITY)) return false;
    w[0] = d / det; w[1] = -b / det; w[2] = -c / det; w[3] = a / det;
    return true;
}

__device__ __forceinline__ bool is_fin(double v) { return fabs(v) < INFINITY; }

}  // namespace

__global__ void __launch_bounds__(WAVE) crx_lqr_design_kernel(const crx_lqr_kparams kp) {
    __shared__ double sm[L_TOTAL];
    const int b = blockIdx.x;
    if (b >= kp.batch) return;
    const int lane = threadIdx.x;
    if (kp.active && kp.active[b] == 0) {
        if (lane == 0) kp.status[b] = CRX_SKIPPED;
        return;
    }
    const int r6 = lane / 6, c6 = lane % 6;           // entry of a 6x6 product, lanes 0..35
    const int l12 = lane - 36;                        // entry of a 6x2 / 2x6 product, lanes 36..47
    double a_in = 0.0, b_in = 0.0;
    if (lane < 36) { a_in = kp.A[(size_t)36 * b + lane]; sm[L_A + lane] = a_in; sm[L_Q + lane] = kp.Q[lane]; sm[L_P + lane] = kp.Q[lane]; }
    if (lane < 12) { b_in = kp.B[(size_t)12 * b + lane]; sm[L_B + lane] = b_in; }
    if (lane < 4) sm[L_R + lane] = kp.R[lane];
    // (L4) a non-finite model never enters the iteration
    bool ok = __ballot(!is_fin(a_in) || !is_fin(b_in)) == 0ull;
    SYNC();

    int status = CRX_MAX_ITER, it = 0;
#pragma unroll 1
    while (ok && it < kp.max_iter) {   // bounded by max_iter whatever the data
        it++;
        // (1) T = A' P, PB = P B
        if (lane < 36) {
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < 6; m++) v += sm[L_A + 6 * m + r6] * sm[L_P + 6 * m + c6];
            sm[L_T + lane] = v;
        } else if (lane < 48) {
            const int r = l12 / 2, a = l12 % 2;
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < 6; m++) v += sm[L_P + 6 * r + m] * sm[L_B + 2 * m + a];
            sm[L_PB + l12] = v;
        }
        SYNC();
        // (2) t1 = (A' P) A (kept by its lane), S = A' (PB) (L2: not (B' P A)'), G = R + B' (PB)
        double t1 = 0.0;
        if (lane < 36) {
#pragma unroll
            for (int m = 0; m < 6; m++) t1 += sm[L_T + 6 * r6 + m] * sm[L_A + 6 * m + c6];
        } else if (lane < 48) {
            const int r = l12 / 2, a = l12 % 2;
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < 6; m++) v += sm[L_A + 6 * m + r] * sm[L_PB + 2 * m + a];
            sm[L_S + l12] = v;
        } else if (lane < 52) {
            const int a = (lane - 48) / 2, c = (lane - 48) % 2;
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < 6; m++) v += sm[L_B + 2 * m + a] * sm[L_PB + 2 * m + c];
            sm[L_G + lane - 48] = sm[L_R + lane - 48] + v;
        }
        SYNC();
        // (3) W = S inv(G)
        double w[4];
        if (!inv2(sm + L_G, w)) { ok = false; break; }
        if (lane < 12) {
            const int r = lane / 2, a = lane % 2;
            sm[L_S2 + lane] = sm[L_S + 2 * r] * (a == 0 ? w[0] : w[1]) + sm[L_S + 2 * r + 1] * (a == 0 ? w[2] : w[3]);
        }
        SYNC();
        // (4) V = W B'
        if (lane < 36) sm[L_V + lane] = sm[L_S2 + 2 * r6] * sm[L_B + 2 * c6] + sm[L_S2 + 2 * r6 + 1] * sm[L_B + 2 * c6 + 1];
        SYNC();
        // (5) T = V P (B' P formed here, separately from A' PB: L2)
        if (lane < 36) {
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < 6; m++) v += sm[L_V + 6 * r6 + m] * sm[L_P + 6 * m + c6];
            sm[L_T + lane] = v;
        }
        SYNC();
        // (6) P' = (t1 - T A) + Q; (L3) strict stop test on the full 6x6 difference; (L1) a passing P' is discarded
        double pn = 0.0;
        bool moved = false, bad = false;
        if (lane < 36) {
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < 6; m++) v += sm[L_T + 6 * r6 + m] * sm[L_A + 6 * m + c6];
            pn = (t1 - v) + sm[L_Q + lane];
            bad = !is_fin(pn);
            moved = !(fabs(pn - sm[L_P + lane]) < kp.eps);
        }
        if (__ballot(bad) != 0ull) { ok = false; break; }
        if (__ballot(moved) == 0ull) { status = CRX_CONVERGED; break; }
        SYNC();   // every read of P above is done
        if (lane < 36) sm[L_P + lane] = pn;
        SYNC();
    }

    // K = ((inv((B' P) B + R) B') P) A from the P in hand
    double kv = 0.0;
    if (ok) {
        if (lane < 12) {
            const int a = lane / 6, c = lane % 6;
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < 6; m++) v += sm[L_B + 2 * m + a] * sm[L_P + 6 * m + c];
            sm[L_PB + lane] = v;
        }
        SYNC();
        if (lane < 4) {
            const int a = lane / 2, c = lane % 2;
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < 6; m++) v += sm[L_PB + 6 * a + m] * sm[L_B + 2 * m + c];
            sm[L_G + lane] = v + sm[L_R + lane];
        }
        SYNC();
        double w[4];
        ok = inv2(sm + L_G, w);
        if (ok) {
            if (lane < 12) {
                const int a = lane / 6, c = lane % 6;
                sm[L_S + lane] = (a == 0 ? w[0] : w[2]) * sm[L_B + 2 * c] + (a == 0 ? w[1] : w[3]) * sm[L_B + 2 * c + 1];
            }
            SYNC();
            if (lane < 12) {
                const int a = lane / 6, c = lane % 6;
                double v = 0.0;
#pragma unroll
                for (int m = 0; m < 6; m++) v += sm[L_S + 6 * a + m] * sm[L_P + 6 * m + c];
                sm[L_S2 + lane] = v;
            }
            SYNC();
            if (lane < 12) {
                const int a = lane / 6, c = lane % 6;
#pragma unroll
                for (int m = 0; m < 6; m++) kv += sm[L_S2 + 6 * a + m] * sm[L_A + 6 * m + c];
            }
            ok = __ballot(lane < 12 && !is_fin(kv)) == 0ull;
        }
    }
    // (L4) no path leaves a finite wrong number
    if (!ok) status = CRX_SINGULAR;
    if (lane < 12) kp.K[(size_t)12 * b + lane] = ok ? kv : NAN;
    if (kp.P && lane < 36) kp.P[(size_t)36 * b + lane] = ok ? sm[L_P + lane] : NAN;
    if (lane == 0) {
        kp.status[b] = status;
        kp.iters[b] = it;
    }
}

__global__ void __launch_bounds__(256) crx_lqr_step_kernel(int batch, const double* __restrict__ K, const double* __restrict__ xcurv,
                                                            const double* __restrict__ xt, double* __restrict__ u) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= batch) return;
    double d[6];
#pragma unroll
    for (int c = 0; c < 6; c++) d[c] = xcurv[(size_t)6 * b + c] - xt[(size_t)6 * b + c];
#pragma unroll
    for (int a = 0; a < 2; a++) {
        double v = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) v += K[(size_t)12 * b + 6 * a + c] * d[c];
        u[(size_t)2 * b + a] = -v;
    }
}

hipError_t crx_launch_lqr_design(const crx_lqr_kparams& kp, hipStream_t st) {
    if (kp.batch == 0) return hipSuccess;
    hipLaunchKernelGGL(crx_lqr_design_kernel, dim3(kp.batch), dim3(WAVE), 0, st, kp);
    return hipGetLastError();
}

hipError_t crx_launch_lqr_step(int batch, const double* K, const double* xcurv, const double* xt, double* u, hipStream_t st) {
    if (batch == 0) return hipSuccess;
    hipLaunchKernelGGL(crx_lqr_step_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, batch, K, xcurv, xt, u);
    return hipGetLastError();
}
