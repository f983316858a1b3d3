// crx_sysid.hip -- batched LTI system identification (system/system_identification.py:4-43 linear_regression), FP64, gfx950
// only, and the PID step of the identification experiment's data loop (control/control.py:15-25 pid).
//
// One fit: W = inv(X'X + lamb I) (X'Y) over the pairs (z, y) = ([x_r | u_r], x_{r+1}) of a group of logs (include/crx.h S1..S5).
// Four launches, no atomics, every sum in a fixed order (crx.h, "Summation"):
//   gram      one 256-thread workgroup per (log, tile) of chunk_rows pairs: each lane streams whole rows (16-B loads) and
//             accumulates the 36 unique entries of z z' and the 48 of z y' in registers, pairs ascending; the waves reduce
//             with crx_wave.h's packed butterflies, then the four waves are added in ascending order -> 84 doubles per tile.
//   solve     one 256-thread workgroup per group: the group's logs are dealt to the lanes in turn, each lane adds its logs'
//             tiles (log ascending, tile ascending), the lanes are reduced as in `gram`.  Lanes 0..7 of wave 0 then hold one
//             row each of X'X + lamb I and of I and run numpy.linalg.inv's algorithm (LAPACK getrf: partial pivoting, first
//             maximum; getrs: the row swaps applied to I, unit-lower then upper triangular solve), then W = inv * (X'Y).
//   residual  the `gram` tiles again: per-column max / min of z'W - y (NaN propagates, as numpy's max does) -> 12 doubles per tile.
//   errfin    one wave per group: max / min over the group's tiles (exact, any order) -> err.
// Workspace: [n_logs * tpl][84] Gram partials, [n_logs * tpl][12] residual partials, [n_groups][48] W, tpl = tiles per log slot.
#include <hip/hip_runtime.h>
#include <math.h>

#if !defined(__HIP_DEVICE_COMPILE__) || defined(__gfx950__)
#else
#error "crx_sysid.hip targets gfx950 (MI355X) only"
#endif

#include "crx_kparams.h"
#include "crx_wave.h"

#define SYSID_THREADS 256
#define SYSID_WAVES (SYSID_THREADS / WAVE)
#define SYSID_NG 84   // 36 unique entries of X'X (upper triangle, row-major) + 48 of X'Y ([8][6] row-major)
#define SYSID_NR 12   // max of the 6 residual columns, then min

namespace {

__device__ __forceinline__ double op_nmax(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double op_nmin(double a, double b) { return (a < b || a != a) ? a : b; }

__device__ __forceinline__ int64_t log_pairs(const crx_sysid_kparams& kp, int l) {
    const int64_t n = kp.log_off[l + 1] - kp.log_off[l] - 1 - kp.first_row;
    return n > 0 ? n : 0;
}
__device__ __forceinline__ int log_tiles(const crx_sysid_kparams& kp, int64_t pairs) {
    const int64_t t = (pairs + kp.chunk - 1) / kp.chunk;
    return t < kp.tpl ? (int)t : kp.tpl;   // never past the log's workspace slot (crx.h: max_log_rows bounds every log)
}
__device__ __forceinline__ void group_logs(const crx_sysid_kparams& kp, int g, int& g0, int& g1) {
    if (kp.grp_off) { g0 = kp.grp_off[g]; g1 = kp.grp_off[g + 1]; } else { g0 = g; g1 = g + 1; }
}

// 84 register partials of one thread -> one value per entry for the workgroup: packed wave butterflies, then the waves in order.
__device__ __forceinline__ void block_sum84(double (&acc)[SYSID_NG], double (*part)[SYSID_NG], double* out) {
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
#pragma unroll
    for (int q = 0; q < SYSID_NG; q += 4) {
        wave_sum4(acc[q], acc[q + 1], acc[q + 2], acc[q + 3]);
        if (lane == 0) { part[w][q] = acc[q]; part[w][q + 1] = acc[q + 1]; part[w][q + 2] = acc[q + 2]; part[w][q + 3] = acc[q + 3]; }
    }
    __syncthreads();
    if (threadIdx.x < SYSID_NG) {
        double s = part[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < SYSID_WAVES; k++) s += part[k][threadIdx.x];
        out[threadIdx.x] = s;
    }
}

__device__ __forceinline__ void load_pair(const crx_sysid_kparams& kp, int64_t r, double (&z)[8], double (&y)[6]) {
    const double2* xr = reinterpret_cast<const double2*>(kp.x + 6 * r);
    const double2 a = xr[0], b = xr[1], c = xr[2], d = xr[3], e = xr[4], f = xr[5];
    const double2 v = reinterpret_cast<const double2*>(kp.u)[r];
    z[0] = a.x; z[1] = a.y; z[2] = b.x; z[3] = b.y; z[4] = c.x; z[5] = c.y; z[6] = v.x; z[7] = v.y;
    y[0] = d.x; y[1] = d.y; y[2] = e.x; y[3] = e.y; y[4] = f.x; y[5] = f.y;
}

__global__ __launch_bounds__(SYSID_THREADS) void sysid_gram_kernel(crx_sysid_kparams kp) {
    __shared__ double part[SYSID_WAVES][SYSID_NG];
    const int l = blockIdx.x / kp.tpl, c = blockIdx.x % kp.tpl;
    const int64_t pairs = log_pairs(kp, l);
    const int64_t p0 = (int64_t)c * kp.chunk;
    if (c >= log_tiles(kp, pairs)) return;   // workgroup-uniform: no tile here
    const int64_t p1 = p0 + kp.chunk < pairs ? p0 + kp.chunk : pairs;
    const int64_t r0 = kp.log_off[l] + kp.first_row;
    double acc[SYSID_NG];
#pragma unroll
    for (int q = 0; q < SYSID_NG; q++) acc[q] = 0.0;
    for (int64_t p = p0 + threadIdx.x; p < p1; p += SYSID_THREADS) {
        double z[8], y[6];
        load_pair(kp, r0 + p, z, y);
        int q = 0;
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int j = i; j < 8; j++) acc[q++] += z[i] * z[j];
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int k = 0; k < 6; k++) acc[36 + 6 * i + k] += z[i] * y[k];
    }
    block_sum84(acc, part, kp.ws_gram + (size_t)blockIdx.x * SYSID_NG);
}

__device__ __forceinline__ int sym_index(int i, int j) {   // (i <= j) -> position in the 36 upper-triangle entries
    return i * 8 - i * (i - 1) / 2 + (j - i);
}

__global__ __launch_bounds__(SYSID_THREADS) void sysid_solve_kernel(crx_sysid_kparams kp) {
    __shared__ double part[SYSID_WAVES][SYSID_NG];
    __shared__ double G[SYSID_NG];
    __shared__ double Wsh[48];
    __shared__ long long cnt[SYSID_THREADS];
    const int g = blockIdx.x;
    int g0, g1;
    group_logs(kp, g, g0, g1);
    double acc[SYSID_NG];
#pragma unroll
    for (int q = 0; q < SYSID_NG; q++) acc[q] = 0.0;
    long long np = 0;
    for (int l = g0 + threadIdx.x; l < g1; l += SYSID_THREADS) {
        const int64_t pairs = log_pairs(kp, l);
        const int nt = log_tiles(kp, pairs);
        np += pairs;
        for (int c = 0; c < nt; c++) {
            const double2* t = reinterpret_cast<const double2*>(kp.ws_gram + ((size_t)l * kp.tpl + c) * SYSID_NG);
#pragma unroll
            for (int q = 0; q < SYSID_NG / 2; q++) {
                const double2 v = t[q];
                acc[2 * q] += v.x;
                acc[2 * q + 1] += v.y;
            }
        }
    }
    cnt[threadIdx.x] = np;
    block_sum84(acc, part, G);
    __syncthreads();
    if (threadIdx.x >= WAVE) return;   // the solve is wave 0's
    const int lane = threadIdx.x;
    long long n_pairs = 0;
    for (int k = 0; k < SYSID_THREADS; k++) n_pairs += cnt[k];
    double* Wg = kp.ws_W + (size_t)g * 48;
    const double nan = __builtin_nan("");
    if (n_pairs == 0) {
        if (lane == 0) { kp.n_pairs[g] = 0; kp.status[g] = CRX_SKIPPED; }
        if (lane < 48) Wg[lane] = nan;
        if (lane < 12) kp.err[(size_t)g * 12 + lane] = nan;
        if (lane < 36) kp.A[(size_t)g * 36 + lane] = nan;
        if (lane < 12) kp.B[(size_t)g * 12 + lane] = nan;
        return;
    }
    // lane i < 8: row i of M = X'X + lamb I and of R = I (lanes 8..63 mirror row 0 and are never read)
    const int i = lane < 8 ? lane : 0;
    double a[8], r[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        a[j] = i <= j ? G[sym_index(i, j)] : G[sym_index(j, i)];
        if (j == i) a[j] += kp.lamb;
        r[j] = j == i ? 1.0 : 0.0;
    }
    bool singular = false;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        // pivot: first row >= k of largest |M[.][k]| (idamax)
        int p = k;
        double best = fabs(lane_f64(a[k], k));
#pragma unroll
        for (int m = k + 1; m < 8; m++) {
            const double v = fabs(lane_f64(a[k], m));
            if (v > best) { best = v; p = m; }
        }
        if (p != k) {
            const int src = lane == k ? p : (lane == p ? k : lane);
#pragma unroll
            for (int j = 0; j < 8; j++) { a[j] = __shfl(a[j], src); r[j] = __shfl(r[j], src); }
        }
        const double piv = lane_f64(a[k], k);
        if (!(piv != 0.0 && isfinite(piv))) singular = true;
        const double rcp = 1.0 / piv;
        double rowk[8];
#pragma unroll
        for (int j = k + 1; j < 8; j++) rowk[j] = lane_f64(a[j], k);
        if (lane > k && lane < 8) {
            const double lik = a[k] * rcp;   // getf2 scales the column by the reciprocal of the pivot
            a[k] = lik;
#pragma unroll
            for (int j = k + 1; j < 8; j++) a[j] -= lik * rowk[j];
        }
    }
    // getrs: L (unit lower) then U, on R = P I
#pragma unroll
    for (int k = 0; k < 8; k++) {
        double rk[8];
#pragma unroll
        for (int j = 0; j < 8; j++) rk[j] = lane_f64(r[j], k);
        if (lane > k && lane < 8) {
#pragma unroll
            for (int j = 0; j < 8; j++) r[j] -= a[k] * rk[j];
        }
    }
#pragma unroll
    for (int k = 7; k >= 0; k--) {
        if (lane == k) {
#pragma unroll
            for (int j = 0; j < 8; j++) r[j] /= a[k];
        }
        double rk[8];
#pragma unroll
        for (int j = 0; j < 8; j++) rk[j] = lane_f64(r[j], k);
        if (lane < k) {
#pragma unroll
            for (int j = 0; j < 8; j++) r[j] -= rk[j] * a[k];
        }
    }
    // W row i = inv row i * (X'Y)
    if (lane < 8) {
#pragma unroll
        for (int c = 0; c < 6; c++) {
            double w = 0.0;
#pragma unroll
            for (int k = 0; k < 8; k++) w += r[k] * G[36 + 6 * k + c];
            Wsh[6 * lane + c] = singular ? nan : w;
        }
    }
    SYNC();
    if (lane < 48) Wg[lane] = Wsh[lane];
    if (lane < 36) kp.A[(size_t)g * 36 + lane] = Wsh[6 * (lane % 6) + lane / 6];          // A = W'[:, 0:6]
    if (lane < 12) kp.B[(size_t)g * 12 + lane] = Wsh[6 * (6 + lane % 2) + lane / 2];      // B = W'[:, 6:8]
    if (singular && lane < 12) kp.err[(size_t)g * 12 + lane] = nan;
    if (lane == 0) { kp.n_pairs[g] = n_pairs; kp.status[g] = singular ? CRX_SINGULAR : CRX_CONVERGED; }
}

__global__ __launch_bounds__(SYSID_THREADS) void sysid_residual_kernel(crx_sysid_kparams kp) {
    __shared__ double part[SYSID_WAVES][SYSID_NR];
    const int l = blockIdx.x / kp.tpl, c = blockIdx.x % kp.tpl;
    const int64_t pairs = log_pairs(kp, l);
    const int64_t p0 = (int64_t)c * kp.chunk;
    if (c >= log_tiles(kp, pairs)) return;
    // the log's group: last g with grp_off[g] <= l (uniform binary search)
    int g = l;
    if (kp.grp_off) {
        int lo = 0, hi = kp.n_groups;   // grp_off[lo] <= l < grp_off[hi] (grp_off[n_groups] = n_logs > l)
        while (hi - lo > 1) {
            const int mid = (lo + hi) / 2;
            if (kp.grp_off[mid] <= l) lo = mid; else hi = mid;
        }
        g = lo;
    }
    if (kp.status[g] != CRX_CONVERGED) return;   // singular: err is NaN already
    const int64_t p1 = p0 + kp.chunk < pairs ? p0 + kp.chunk : pairs;
    const int64_t r0 = kp.log_off[l] + kp.first_row;
    const double* Wg = kp.ws_W + (size_t)g * 48;
    double W[48];
#pragma unroll
    for (int q = 0; q < 48; q++) W[q] = Wg[q];
    double mx[6], mn[6];
#pragma unroll
    for (int k = 0; k < 6; k++) { mx[k] = -INFINITY; mn[k] = INFINITY; }
    for (int64_t p = p0 + threadIdx.x; p < p1; p += SYSID_THREADS) {
        double z[8], y[6];
        load_pair(kp, r0 + p, z, y);
#pragma unroll
        for (int k = 0; k < 6; k++) {
            double e = 0.0;
#pragma unroll
            for (int j = 0; j < 8; j++) e += z[j] * W[6 * j + k];
            e -= y[k];
            mx[k] = op_nmax(mx[k], e);
            mn[k] = op_nmin(mn[k], e);
        }
    }
    WAVE_REDUCE4(mx[0], mx[1], mx[2], mx[3], op_nmax);
    WAVE_REDUCE2(mx[4], mx[5], op_nmax);
    WAVE_REDUCE4(mn[0], mn[1], mn[2], mn[3], op_nmin);
    WAVE_REDUCE2(mn[4], mn[5], op_nmin);
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; k++) { part[w][k] = mx[k]; part[w][6 + k] = mn[k]; }
    }
    __syncthreads();
    if (threadIdx.x < SYSID_NR) {
        const int k = threadIdx.x;
        double v = part[0][k];
#pragma unroll
        for (int m = 1; m < SYSID_WAVES; m++) v = k < 6 ? op_nmax(v, part[m][k]) : op_nmin(v, part[m][k]);
        kp.ws_res[(size_t)blockIdx.x * SYSID_NR + k] = v;
    }
}

__global__ __launch_bounds__(WAVE) void sysid_errfin_kernel(crx_sysid_kparams kp) {
    const int g = blockIdx.x;
    if (kp.status[g] != CRX_CONVERGED) return;   // NaN written by the solve kernel
    int g0, g1;
    group_logs(kp, g, g0, g1);
    double mx[6], mn[6];
#pragma unroll
    for (int k = 0; k < 6; k++) { mx[k] = -INFINITY; mn[k] = INFINITY; }
    for (int l = g0 + (int)threadIdx.x; l < g1; l += WAVE) {
        const int nt = log_tiles(kp, log_pairs(kp, l));
        for (int c = 0; c < nt; c++) {
            const double* t = kp.ws_res + ((size_t)l * kp.tpl + c) * SYSID_NR;
#pragma unroll
            for (int k = 0; k < 6; k++) { mx[k] = op_nmax(mx[k], t[k]); mn[k] = op_nmin(mn[k], t[6 + k]); }
        }
    }
    WAVE_REDUCE4(mx[0], mx[1], mx[2], mx[3], op_nmax);
    WAVE_REDUCE2(mx[4], mx[5], op_nmax);
    WAVE_REDUCE4(mn[0], mn[1], mn[2], mn[3], op_nmin);
    WAVE_REDUCE2(mn[4], mn[5], op_nmin);
    const int lane = threadIdx.x;
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) { if (lane == k) v = mx[k]; if (lane == 6 + k) v = mn[k]; }
    if (lane < SYSID_NR) kp.err[(size_t)g * 12 + lane] = v;   // err[g][0][:] = max, err[g][1][:] = min
}

__global__ void pid_log_kernel(crx_pid_kparams kp) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= kp.batch) return;
    const double* x = kp.xcurv + 6 * (size_t)b;
    if (kp.row >= 0) {
        double* xl = kp.x_log + ((size_t)b * kp.T + kp.row) * 6;
        double* ul = kp.u_log + ((size_t)b * kp.T + kp.row) * 2;
#pragma unroll
        for (int k = 0; k < 6; k++) xl[k] = x[k];
        ul[0] = kp.u_prev[2 * (size_t)b];
        ul[1] = kp.u_prev[2 * (size_t)b + 1];
    }
    if (kp.u_next) {
        // control.pid: u[0] = -0.6 * (ey - eyt) - 0.9 * epsi, u[1] = 1.5 * (vt - vx), rounded as numpy does (no contraction)
        kp.u_next[2 * (size_t)b] = __dsub_rn(__dmul_rn(-0.6, __dsub_rn(x[5], kp.eyt[b])), __dmul_rn(0.9, x[3]));
        kp.u_next[2 * (size_t)b + 1] = __dmul_rn(1.5, __dsub_rn(kp.vt[b], x[0]));
    }
}

}  // namespace

hipError_t crx_launch_sysid(const crx_sysid_kparams& kp, hipStream_t st) {
    if (kp.n_groups == 0) return hipSuccess;
    const unsigned tiles = (unsigned)kp.n_logs * (unsigned)kp.tpl;
    if (tiles) hipLaunchKernelGGL(sysid_gram_kernel, dim3(tiles), dim3(SYSID_THREADS), 0, st, kp);
    hipLaunchKernelGGL(sysid_solve_kernel, dim3(kp.n_groups), dim3(SYSID_THREADS), 0, st, kp);
    if (tiles) hipLaunchKernelGGL(sysid_residual_kernel, dim3(tiles), dim3(SYSID_THREADS), 0, st, kp);
    hipLaunchKernelGGL(sysid_errfin_kernel, dim3(kp.n_groups), dim3(WAVE), 0, st, kp);
    return hipGetLastError();
}

hipError_t crx_launch_pid_log(const crx_pid_kparams& kp, hipStream_t st) {
    if (kp.batch == 0) return hipSuccess;
    hipLaunchKernelGGL(pid_log_kernel, dim3((kp.batch + 255) / 256), dim3(256), 0, st, kp);
    return hipGetLastError();
}
