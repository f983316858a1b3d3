// crx_debug_wave.hip -- diagnostics (crx_debug_wave_prim, not in crx.h): every primitive of crx_wave.h on host data, one 64-lane workgroup
// per case, so that tests/test_gpu_wave_prims.py can pin each of them against exact arithmetic (tests/wave_model.py).  Nothing here is on a
// product path.  The kernels index memory from blockIdx / threadIdx / the launch parameters only and contain no data-dependent loop: no
// input VALUE can fault or hang them (the launch parameters are validated on the host before anything is launched).
//
// Layouts (doubles, per case; `in` at case * in_stride, `out` at case * out_stride; every array below is [64], lane-indexed, unless stated):
//   op 1 LANES   in  x, y                     out lane_f64(x, case & 63) | ROW_REDUCE(x, +) per lane | swap32(x, y): x', y' | swap16(x, y): x', y'
//   op 2 SUMS    in  a, b, c, d               out wave_sum(a) | wave_prod(b) | wave_sum2(a, b): a', b' | wave_sum4(a, b, c, d): a', b', c', d'
//   op 3 MAXS    in  a, b, c, d               out wave_max(a) | wave_min(b) | wave_max2(c, d): c', d' | wave_max4(a, b, c, d): a', b', c', d'
//   op 4 ROWDOT  in  x, x2, acc, m[9], sent   out row_dot<CNT, FIRST>      iarg: [0] instantiation (kRowDot below), [1] NZ (0: full EXEC, else inside
//                                                 `if (lane < NZ)`, the other lanes return sent), [2] mode: 0 x as loaded, 1 x = x + x2 (a VALU result
//                                                 in front of the s_nop), 2 chained: the result of the first dot product is x AND acc of a second one
//   op 5 HALFROW in  x, x2, m[6]              out halfrow_dot6(x, m, lane & 8)                           iarg: [2] mode 0 / 1 as above
//   op 6 SCANS   in  x                        out excl_prefix | excl_suffix
//   op 7 RECIP   in  x                        out frcp | frsqrt | log2_fast
//   op 8 LOGACC  in  v[6], other              out wave_total | wave_total_with(other) | other'           iarg: [0] factors per lane, 1 .. 6
//   op 9 WRAPS   in  s, L                     out wrap_above | wrap_below
//   op 10 CHOL   in  image[total], b[2]       out image[total] after l_chol (+ l_backsub), x[2], ok[64]  iarg: n, extra, LD, base, inv, inv_st, total, NR
#include <hip/hip_runtime.h>

#include "crx_wave.h"
#include "../../include/crx.h"

namespace {

constexpr int CHOL_MAX = 6144;      // doubles of LDS image (48 KB)

struct Args { const double* in; double* out; long is, os; int a[8]; };

// the <CNT, FIRST> pairs the solver kernels form (NX = 6 .. 9, PVF = 8, NU = 2 .. 5) and three extremes
constexpr int kRowDot[12][2] = {{6, 0}, {7, 0}, {8, 0}, {9, 0}, {7, 8}, {2, 6}, {3, 7}, {4, 8}, {5, 9}, {2, 14}, {9, 7}, {8, 8}};

template <int CNT, int FIRST>
__device__ __forceinline__ double rowdot_case(const double* in, int lane, int nz, int mode) {
    double m[CNT];
#pragma unroll
    for (int i = 0; i < CNT; i++) m[i] = in[(3 + i) * 64 + lane];
    const double x0 = in[lane], x2 = in[64 + lane], acc = in[128 + lane];
    double r = in[12 * 64 + lane];
    if (nz == 0) {
        if (mode == 0) r = row_dot<CNT, FIRST>(x0, m, acc);
        else if (mode == 1) r = row_dot<CNT, FIRST>(x0 + x2, m, acc);
        else { const double first = row_dot<CNT, FIRST>(x0, m, acc); r = row_dot<CNT, FIRST>(first, m, first); }
    } else if (lane < nz) {
        if (mode == 0) r = row_dot<CNT, FIRST>(x0, m, acc);
        else if (mode == 1) r = row_dot<CNT, FIRST>(x0 + x2, m, acc);
        else { const double first = row_dot<CNT, FIRST>(x0, m, acc); r = row_dot<CNT, FIRST>(first, m, first); }
    }
    return r;
}

__global__ void __launch_bounds__(WAVE) crx_debug_lanes_kernel(Args g) {
    const int lane = threadIdx.x;
    const double* in = g.in + (long)blockIdx.x * g.is;
    double* out = g.out + (long)blockIdx.x * g.os;
    const double x = in[lane], y = in[64 + lane];
    out[lane] = lane_f64(x, blockIdx.x & 63);
    double r = x;
    ROW_REDUCE(r, op_add)
    out[64 + lane] = r;
    double a = x, b = y;
    swap32_f64(a, b);
    out[128 + lane] = a; out[192 + lane] = b;
    a = x; b = y;
    swap16_f64(a, b);
    out[256 + lane] = a; out[320 + lane] = b;
}

template <bool MAXS>
__global__ void __launch_bounds__(WAVE) crx_debug_reduce_all_kernel(Args g) {
    const int lane = threadIdx.x;
    const double* in = g.in + (long)blockIdx.x * g.is;
    double* out = g.out + (long)blockIdx.x * g.os;
    const double a = in[lane], b = in[64 + lane], c = in[128 + lane], d = in[192 + lane];
    double p0, p1, q0 = a, q1 = b, q2 = c, q3 = d;
    if constexpr (MAXS) {
        out[lane] = wave_max(a); out[64 + lane] = wave_min(b);
        p0 = c; p1 = d; wave_max2(p0, p1); wave_max4(q0, q1, q2, q3);
    } else {
        out[lane] = wave_sum(a); out[64 + lane] = wave_prod(b);
        p0 = a; p1 = b; wave_sum2(p0, p1); wave_sum4(q0, q1, q2, q3);
    }
    out[128 + lane] = p0; out[192 + lane] = p1;
    out[256 + lane] = q0; out[320 + lane] = q1; out[384 + lane] = q2; out[448 + lane] = q3;
}

__global__ void __launch_bounds__(WAVE) crx_debug_rowdot_kernel(Args g) {
    const int lane = threadIdx.x;
    const double* in = g.in + (long)blockIdx.x * g.is;
    double* out = g.out + (long)blockIdx.x * g.os;
    const int nz = g.a[1], mode = g.a[2];
    double r = 0.0;
    switch (g.a[0]) {
    case 0: r = rowdot_case<6, 0>(in, lane, nz, mode); break;
    case 1: r = rowdot_case<7, 0>(in, lane, nz, mode); break;
    case 2: r = rowdot_case<8, 0>(in, lane, nz, mode); break;
    case 3: r = rowdot_case<9, 0>(in, lane, nz, mode); break;
    case 4: r = rowdot_case<7, 8>(in, lane, nz, mode); break;
    case 5: r = rowdot_case<2, 6>(in, lane, nz, mode); break;
    case 6: r = rowdot_case<3, 7>(in, lane, nz, mode); break;
    case 7: r = rowdot_case<4, 8>(in, lane, nz, mode); break;
    case 8: r = rowdot_case<5, 9>(in, lane, nz, mode); break;
    case 9: r = rowdot_case<2, 14>(in, lane, nz, mode); break;
    case 10: r = rowdot_case<9, 7>(in, lane, nz, mode); break;
    default: r = rowdot_case<8, 8>(in, lane, nz, mode); break;
    }
    out[lane] = r;
}

__global__ void __launch_bounds__(WAVE) crx_debug_halfrow_kernel(Args g) {
    const int lane = threadIdx.x;
    const double* in = g.in + (long)blockIdx.x * g.is;
    double* out = g.out + (long)blockIdx.x * g.os;
    double m[6];
#pragma unroll
    for (int i = 0; i < 6; i++) m[i] = in[(2 + i) * 64 + lane];
    const double x0 = in[lane], x2 = in[64 + lane];
    const bool upper = (lane & 8) != 0;
    out[lane] = g.a[2] == 0 ? halfrow_dot6(x0, m, upper) : halfrow_dot6(x0 + x2, m, upper);
}

__global__ void __launch_bounds__(WAVE) crx_debug_scan_kernel(Args g) {
    const int lane = threadIdx.x;
    const double x = g.in[(long)blockIdx.x * g.is + lane];
    double* out = g.out + (long)blockIdx.x * g.os;
    out[lane] = excl_prefix(x, lane);
    out[64 + lane] = excl_suffix(x, lane);
}

__global__ void __launch_bounds__(WAVE) crx_debug_recip_kernel(Args g) {
    const int lane = threadIdx.x;
    const double x = g.in[(long)blockIdx.x * g.is + lane];
    double* out = g.out + (long)blockIdx.x * g.os;
    out[lane] = frcp(x);
    out[64 + lane] = frsqrt(x);
    out[128 + lane] = log2_fast(x);
}

__global__ void __launch_bounds__(WAVE) crx_debug_logacc_kernel(Args g) {
    const int lane = threadIdx.x;
    const double* in = g.in + (long)blockIdx.x * g.is;
    double* out = g.out + (long)blockIdx.x * g.os;
    const int k = g.a[0];
    LogAcc l0, l1;
#pragma unroll
    for (int i = 0; i < 6; i++)
        if (i < k) { const double v = in[i * 64 + lane]; l0.mul(v); l1.mul(v); }
    double other = in[6 * 64 + lane];
    out[lane] = l0.wave_total();
    out[64 + lane] = l1.wave_total_with(other);
    out[128 + lane] = other;
}

__global__ void __launch_bounds__(WAVE) crx_debug_wrap_kernel(Args g) {
    const int lane = threadIdx.x;
    const double* in = g.in + (long)blockIdx.x * g.is;
    double* out = g.out + (long)blockIdx.x * g.os;
    const double s = in[lane], L = in[64 + lane];
    out[lane] = wrap_above(s, L);
    out[64 + lane] = wrap_below(s, L);
}

__global__ void __launch_bounds__(WAVE) crx_debug_chol_kernel(Args g) {
    __shared__ double sm[CHOL_MAX];
    const int lane = threadIdx.x;
    const double* in = g.in + (long)blockIdx.x * g.is;
    double* out = g.out + (long)blockIdx.x * g.os;
    const int n = g.a[0], extra = g.a[1], LD = g.a[2], base = g.a[3], inv = g.a[4], inv_st = g.a[5], total = g.a[6], nr = g.a[7];
    for (int i = lane; i < total; i += WAVE) sm[i] = in[i];
    SYNC();
    double b[2] = {in[total + lane], in[total + 64 + lane]};
    const int ok = l_chol(sm, base, LD, inv, n, extra, lane, inv_st);
    SYNC();
    if (ok) {
        if (nr == 1) l_backsub<1>(sm, base, LD, inv, n, lane, b, inv_st);
        else l_backsub<2>(sm, base, LD, inv, n, lane, b, inv_st);
    }
    SYNC();
    for (int i = lane; i < total; i += WAVE) out[i] = sm[i];
    out[total + lane] = b[0];
    out[total + 64 + lane] = b[1];
    out[total + 128 + lane] = (double)ok;
}

}  // namespace

extern "C" int crx_debug_wave_prim(int op, int n_cases, const double* in, long in_stride, double* out, long out_stride, const int* iarg) {
    if (!in || !out || n_cases < 1 || n_cases > (1 << 20)) return CRX_ERR_ARG;
    Args g{};
    for (int i = 0; i < 8; i++) g.a[i] = iarg ? iarg[i] : 0;
    long need_in = 0, need_out = 0;
    switch (op) {
    case 1: need_in = 128; need_out = 384; break;
    case 2: case 3: need_in = 256; need_out = 512; break;
    case 4:
        need_in = 13 * 64; need_out = 64;
        if (g.a[0] < 0 || g.a[0] > 11 || g.a[2] < 0 || g.a[2] > 2) return CRX_ERR_ARG;
        // EXEC must cover the lanes read (crx_wave.h): a predicated region has to hold lanes FIRST .. FIRST + CNT - 1
        if (g.a[1] != 0 && (g.a[1] > 16 || g.a[1] < kRowDot[g.a[0]][0] + kRowDot[g.a[0]][1])) return CRX_ERR_ARG;
        break;
    case 5: need_in = 8 * 64; need_out = 64; if (g.a[2] < 0 || g.a[2] > 1) return CRX_ERR_ARG; break;
    case 6: need_in = 64; need_out = 128; break;
    case 7: need_in = 64; need_out = 192; break;
    case 8: need_in = 7 * 64; need_out = 192; if (g.a[0] < 1 || g.a[0] > 6) return CRX_ERR_ARG; break;
    case 9: need_in = 128; need_out = 128; break;
    case 10: {
        const int n = g.a[0], extra = g.a[1], LD = g.a[2], base = g.a[3], inv = g.a[4], inv_st = g.a[5], total = g.a[6], nr = g.a[7];
        if (n < 1 || extra < 0 || n + extra > 64 || LD < n + 1 || LD > 128 || base < 0 || inv < 0 || inv_st < 1 || total < 1 || total > CHOL_MAX ||
            (nr != 1 && nr != 2))
            return CRX_ERR_ARG;
        // the panel loop reads (does not use) rows and columns up to 4 * ceil(n / 4) - 1 of every row it touches
        const int n4 = (n + 3) / 4 * 4, rows = n + extra > n4 ? n + extra : n4;
        if ((long)base + (long)rows * LD + 4 > total || (long)inv + (long)(n - 1) * inv_st >= total) return CRX_ERR_ARG;
        need_in = total + 128; need_out = total + 192;
        break;
    }
    default: return CRX_ERR_ARG;
    }
    if (in_stride < need_in || out_stride < need_out) return CRX_ERR_ARG;
    const size_t nin = (size_t)n_cases * in_stride * sizeof(double), nout = (size_t)n_cases * out_stride * sizeof(double);
    double *din = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc(&din, nin);
    if (e == hipSuccess) e = hipMalloc(&dout, nout);
    if (e == hipSuccess) e = hipMemcpy(din, in, nin, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0xFF, nout);      // what a kernel does not write comes back as NaN
    if (e == hipSuccess) {
        g.in = din; g.out = dout; g.is = in_stride; g.os = out_stride;
        const dim3 grid(n_cases), block(WAVE);
        switch (op) {
        case 1: hipLaunchKernelGGL(crx_debug_lanes_kernel, grid, block, 0, 0, g); break;
        case 2: hipLaunchKernelGGL(crx_debug_reduce_all_kernel<false>, grid, block, 0, 0, g); break;
        case 3: hipLaunchKernelGGL(crx_debug_reduce_all_kernel<true>, grid, block, 0, 0, g); break;
        case 4: hipLaunchKernelGGL(crx_debug_rowdot_kernel, grid, block, 0, 0, g); break;
        case 5: hipLaunchKernelGGL(crx_debug_halfrow_kernel, grid, block, 0, 0, g); break;
        case 6: hipLaunchKernelGGL(crx_debug_scan_kernel, grid, block, 0, 0, g); break;
        case 7: hipLaunchKernelGGL(crx_debug_recip_kernel, grid, block, 0, 0, g); break;
        case 8: hipLaunchKernelGGL(crx_debug_logacc_kernel, grid, block, 0, 0, g); break;
        case 9: hipLaunchKernelGGL(crx_debug_wrap_kernel, grid, block, 0, 0, g); break;
        default: hipLaunchKernelGGL(crx_debug_chol_kernel, grid, block, 0, 0, g); break;
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, nout, hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return e == hipSuccess ? CRX_OK : CRX_ERR_HIP;
}
