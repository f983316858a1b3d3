// crx_api.hip -- the C ABI of libcrx (include/crx.h) on top of the gfx950 kernels.
//
// Host-pointer entry points stage through library-owned, grow-only device buffers on one private
// stream and block; *_dev entry points only enqueue on the caller's stream.  There is no CPU
// path in this library: without a HIP device every solve entry point fails with CRX_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <dlfcn.h>

#include <chrono>
#include <mutex>
#include <vector>

// RCCL: types only -- the entry points are resolved at run time (rccl_bind), libcrx does not link librccl.  A ROCm install without
// the RCCL development headers still builds the single-GPU library: the handful of types the five entry points need are declared
// here then (the stable NCCL 2 ABI: opaque communicator, 128-byte id, int-valued enums)
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclUint8 = 1, ncclInt32 = 2, ncclUint32 = 3, ncclInt64 = 4, ncclUint64 = 5, ncclFloat16 = 6, ncclFloat32 = 7, ncclFloat64 = 8 } ncclDataType_t;
}
#endif

#include "crx_kparams.h"

namespace {

thread_local char g_err[512] = "";
std::mutex g_mu;
int g_device = -1;
bool g_init = false;
hipStream_t g_stream = nullptr;

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return fail(CRX_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

// grow-only buffer over one allocate / free pair: device memory, or pinned host memory
struct DevMem {
    static constexpr const char* name = "hipMalloc";
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t release(void* p) { return hipFree(p); }
};
struct PinMem {
    static constexpr const char* name = "hipHostMalloc";
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t release(void* p) { return hipHostFree(p); }
};
template <typename Mem>
struct Buf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        release();
        size_t want = bytes + bytes / 2 + 256;
        hipError_t e = Mem::alloc(&p, want);
        if (e != hipSuccess) return fail(CRX_ERR_HIP, "%s(%zu): %s", Mem::name, want, hipGetErrorString(e));
        cap = want;
        return 0;
    }
    void release() {
        if (p) (void)Mem::release(p);
        p = nullptr;
        cap = 0;
    }
};
using DevBuf = Buf<DevMem>;
using PinBuf = Buf<PinMem>;
DevBuf g_in, g_out;  // staging for the host-pointer entry points
// pinned host mirrors of g_in / g_out: a host-pointer call gathers ALL its inputs into one pinned block
// (one H2D copy), and scatters its outputs from one pinned block (one D2H copy) -- a batch-1 control step
// is launch-latency bound, and a dozen separate small copies cost more than the solve itself
PinBuf g_hin, g_hout;
DevBuf g_trace;
int g_poison = 0;
int g_kkt_unscaled = 0;
int g_spec = 0;    // diagnostics (crx_debug_speculation): 0 = never (default), 1 = wherever the two-wave instantiation exists, 2 = that kernel with its second wave idle
int g_trace_rows = 0, g_trace_problem = 0;

int ensure_init() {
    if (g_init) return 0;
    return fail(CRX_ERR_NOT_INIT, "crx_init() has not been called (or failed)");
}

using arr = const void*;   // an array argument of which a check only asks whether it is there
template <typename... P>
bool any_null(const P*... p) { return (... || !p); }

// staging plan of one host-pointer call.  The call site names each array ONCE -- in / out / inout / scratch with the host
// pointer and the element count -- and keeps the handle.  up() lays the arrays out, each 256-byte aligned: the inputs in g_in;
// in g_out first the in/outs, then the outputs, last the scratch, so that one H2D copy covers the in/outs and the one D2H copy
// stops in front of the scratch.  It sizes the four buffers from that layout, gathers into the pinned mirrors and uploads.
// The buffers may move when they grow, so sg[handle] is the device address only AFTER up().  down() copies back and scatters.
struct Stage {
    enum Kind { IN, INOUT, OUT, SCRATCH };
    template <typename T>
    struct Ref { int i = -1; };   // -1: an array this call does not use; sg[ref] is NULL
    struct Slot { Kind kind; const void* src; void* dst; size_t bytes, off; };
    static constexpr int MAX_SLOTS = 24;
    Slot slots[MAX_SLOTS];
    int n = 0;
    bool overrun = false;
    size_t end[4] = {0, 0, 0, 0};   // bytes of g_in up to its last input; of g_out up to its last in/out, output, scratch

    template <typename T>
    Ref<T> add(Kind kind, const T* src, T* dst, size_t count) {
        if (n == MAX_SLOTS) { overrun = true; return {}; }   // reported by up(), before anything is copied or launched
        slots[n] = Slot{kind, src, dst, count * sizeof(T), 0};
        return Ref<T>{n++};
    }
    template <typename T>
    Ref<T> in(const T* src, size_t count) { return add(IN, src, (T*)nullptr, count); }   // src may be NULL (array not used by this call): zero-filled
    template <typename T>
    Ref<T> out(T* host, size_t count) { return add(OUT, (const T*)nullptr, host, count); }   // host may be NULL (result not wanted)
    template <typename T>
    Ref<T> inout(T* host, size_t count) { return add(INOUT, (const T*)host, host, count); }   // the kernel updates the caller's data in place
    Ref<char> scratch(size_t bytes) { return add(SCRATCH, (const char*)nullptr, (char*)nullptr, bytes); }   // device bytes without a host side
    template <typename T>
    T* operator[](Ref<T> r) const {
        return r.i < 0 ? nullptr : (T*)((char*)(slots[r.i].kind == IN ? g_in.p : g_out.p) + slots[r.i].off);
    }

    int up(hipStream_t st) {
        if (overrun) return fail(CRX_ERR_ARG, "internal: more than %d staged arrays in one call", MAX_SLOTS);
        size_t cur = 0;
        for (int k = IN; k <= SCRATCH; k++) {
            if (k == INOUT) cur = 0;   // g_out starts here
            for (int i = 0; i < n; i++)
                if (slots[i].kind == k) {
                    slots[i].off = cur = (cur + 255) & ~size_t(255);
                    cur += slots[i].bytes;
                }
            end[k] = cur;
        }
        if (int rc = g_in.ensure(end[IN])) return rc;
        if (int rc = g_hin.ensure(end[IN])) return rc;
        if (int rc = g_out.ensure(end[SCRATCH])) return rc;
        if (int rc = g_hout.ensure(end[OUT])) return rc;
        for (int i = 0; i < n; i++) {
            const Slot& s = slots[i];
            if (s.kind > INOUT || !s.bytes) continue;
            char* pin = (char*)(s.kind == IN ? g_hin.p : g_hout.p) + s.off;
            if (s.src) memcpy(pin, s.src, s.bytes); else memset(pin, 0, s.bytes);
        }
        if (end[IN]) HIP_TRY(hipMemcpyAsync(g_in.p, g_hin.p, end[IN], hipMemcpyHostToDevice, st));
        if (end[INOUT]) HIP_TRY(hipMemcpyAsync(g_out.p, g_hout.p, end[INOUT], hipMemcpyHostToDevice, st));
        return 0;
    }
    int down(hipStream_t st) {
        if (end[OUT]) HIP_TRY(hipMemcpyAsync(g_hout.p, g_out.p, end[OUT], hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int i = 0; i < n; i++)
            if (slots[i].dst && slots[i].bytes) memcpy(slots[i].dst, (char*)g_hout.p + slots[i].off, slots[i].bytes);
        return 0;
    }
};

int check_opts(const crx_ipm_opts& o) {
    if (!(o.tol > 0) || o.max_iter < 1 || !(o.mu_init > 0) || !(o.tau_min > 0 && o.tau_min < 1) ||
        !(o.slack_push > 0) || !(o.kappa_mu > 0 && o.kappa_mu < 1) || !(o.theta_mu > 1) || !(o.grad_scale_max > 0) ||
        o.slack_start < 0 || o.slack_start > 3 || !(o.dual_inf_tol > 0) || !(o.constr_viol_tol > 0) || !(o.compl_inf_tol > 0) || o.stall_iters < 1 || o.qp_method < 0 || o.qp_method > 1)
        return fail(CRX_ERR_ARG, "invalid crx_ipm_opts (a descriptor built for libcrx <= 0.3.x? crx_ipm_opts grew in 0.2 and in 0.4: include/crx.h)");
    return 0;
}

// reach of one state coordinate under the boxed inputs: gain[j] = sum_{m<j} |e_row' A^m B| (delta_max, a_max)' for j = 0..n;
// rows (may be NULL): rows[j] = e_row' A^j
void reach_bound(const double* A, const double* B, double delta_max, double a_max, int row, int n, double* gain, double (*rows)[6]) {
    double w[6] = {0, 0, 0, 0, 0, 0}, acc = 0.0;
    w[row] = 1.0;
    gain[0] = 0.0;
    if (rows) memcpy(rows[0], w, sizeof(w));
    for (int j = 1; j <= n; j++) {
        double v0 = 0.0, v1 = 0.0, wn[6] = {0, 0, 0, 0, 0, 0};
        for (int i = 0; i < 6; i++) { v0 += w[i] * B[i * 2]; v1 += w[i] * B[i * 2 + 1]; }
        acc += fabs(v0) * delta_max + fabs(v1) * a_max;
        gain[j] = acc;
        for (int a = 0; a < 6; a++)
            for (int i = 0; i < 6; i++) wn[a] += w[i] * A[i * 6 + a];
        memcpy(w, wn, sizeof(w));
        if (rows) memcpy(rows[j], w, sizeof(w));
    }
}

// own_model = false: the launch brings one model per problem (crx_planner_solve_models*), d->A and d->B are not read
int fill_planner(crx_kparams& kp, const crx_planner_desc* d, int batch, bool own_model = true) {
    if (!d) return fail(CRX_ERR_ARG, "desc is NULL");
    if (d->N < 3 || d->N > CRX_MAX_N) return fail(CRX_ERR_ARG, "N=%d outside [3,%d]", d->N, CRX_MAX_N);
    if (batch < 0) return fail(CRX_ERR_ARG, "batch < 0");
    if (int rc = check_opts(d->opts)) return rc;
    memset(&kp, 0, sizeof(kp));
    kp.N = d->N; kp.batch = batch; kp.mode = 0; kp.n_obs_max = 0; kp.degree = 6;
    memcpy(kp.A, d->A, sizeof(kp.A)); memcpy(kp.B, d->B, sizeof(kp.B));
    kp.wq[4] = d->w_ref; kp.wq[5] = d->w_ref;
    kp.w_dey = d->w_dey; kp.w_prog = d->w_prog; kp.w_slack = 0.0;
    kp.delta_max = d->delta_max; kp.a_max = d->a_max; kp.v_min = -INFINITY; kp.v_max = d->vx_max; kp.ey_max = INFINITY;
    kp.alpha = 0.0; kp.margin = 0.0; kp.l_sum = 1.0; kp.w_sum = 1.0;
    kp.dt_ref = d->dt_ref; kp.fallback_gain = d->fallback_gain; kp.opts = d->opts;
    // reachability screen (crx_kernels.hip, set-up): the reach of ey at stages 0..N-1 and the rows of its free response
    kp.reach_screen = d->opts.reach_screen ? 1 : 0;
    if (own_model) reach_bound(d->A, d->B, d->delta_max, d->a_max, 5, d->N - 1, kp.reach_gain, kp.reach_row);
    return 0;
}

int fill_cbf(crx_kparams& kp, const crx_cbf_desc* d, int batch) {
    if (!d) return fail(CRX_ERR_ARG, "desc is NULL");
    if (d->N < 3 || d->N > CRX_MAX_N) return fail(CRX_ERR_ARG, "N=%d outside [3,%d]", d->N, CRX_MAX_N);
    if (d->n_obs_max < 0 || d->n_obs_max > CRX_MAX_OBS) return fail(CRX_ERR_ARG, "n_obs_max=%d outside [0,%d]", d->n_obs_max, CRX_MAX_OBS);
    if (d->degree < 2 || d->degree > 8 || (d->degree & 1)) return fail(CRX_ERR_ARG, "degree must be 2, 4, 6 or 8");
    if (batch < 0) return fail(CRX_ERR_ARG, "batch < 0");
    if (!(d->alpha > 0.0 && d->alpha <= 1.0)) return fail(CRX_ERR_ARG, "alpha outside (0,1]");
    if (int rc = check_opts(d->opts)) return rc;
    memset(&kp, 0, sizeof(kp));
    kp.N = d->N; kp.batch = batch; kp.mode = 1; kp.per_stage_target = d->per_stage_target ? 1 : 0;
    kp.n_obs_max = d->n_obs_max; kp.degree = d->degree;
    memcpy(kp.A, d->A, sizeof(kp.A)); memcpy(kp.B, d->B, sizeof(kp.B));
    memcpy(kp.wq, d->Q, sizeof(kp.wq)); kp.wr[0] = d->R[0]; kp.wr[1] = d->R[1];
    kp.w_dey = 0.0; kp.w_prog = 0.0; kp.w_slack = d->w_slack;
    kp.delta_max = d->delta_max; kp.a_max = d->a_max; kp.v_min = d->v_min; kp.v_max = d->v_max; kp.ey_max = d->ey_max;
    kp.alpha = d->alpha; kp.margin = d->margin; kp.l_sum = d->l_sum; kp.w_sum = d->w_sum;
    kp.dt_ref = 0.1; kp.fallback_gain = 1.1; kp.opts = d->opts;
    // reach of s and ey at stages 0..N under the boxed inputs (crx_kernels.hip: slack start)
    kp.slack_start = d->opts.slack_start;
    reach_bound(d->A, d->B, d->delta_max, d->a_max, 4, d->N, kp.reach_s, nullptr);
    reach_bound(d->A, d->B, d->delta_max, d->a_max, 5, d->N, kp.reach_gain, nullptr);
    return 0;
}

int launched(hipError_t e, const char* what) {
    return e == hipSuccess ? CRX_OK : fail(CRX_ERR_HIP, "%s launch: %s", what, hipGetErrorString(e));
}

// the diagnostics switches (crx_trace_enable, crx_debug_poison_lds, crx_debug_kkt_unscaled) of the following launch.  A negative
// trace_rows asks for the Riccati sub-phase cycles, which only the planner / CBF kernel records; so does kkt_unscaled
void apply_diagnostics(crx_kparams& kp) {
    if (g_trace_rows != 0) { kp.trace = (double*)g_trace.p; kp.trace_problem = g_trace_problem; kp.trace_rows = g_trace_rows; }
    kp.poison = g_poison;
    kp.kkt_unscaled = g_kkt_unscaled;
}
void apply_diagnostics(crx_lmpc_kparams& kp) {
    if (g_trace_rows > 0) { kp.trace = (double*)g_trace.p; kp.trace_problem = g_trace_problem; kp.trace_rows = g_trace_rows; }
    kp.poison = g_poison;
}

// mdl: one LTI model per problem (crx_cbf_solve_models_dev; model_A, model_B, model_reach all set) -- NULL: the descriptor's model for all
int launch_solve(const crx_kparams& kp, int tmpl, hipStream_t st, const crx_kparams_models* mdl = nullptr) {
    crx_kparams kq = kp;
    apply_diagnostics(kq);
    size_t lds = crx_solve_lds_bytes(kp.N, tmpl);
    if (lds > 160 * 1024) return fail(CRX_ERR_ARG, "N=%d with %d obstacles needs %zu B of LDS (> 160 KiB)", kp.N, tmpl, lds);
    if (mdl) {   // (the two-wave kernels have no per-problem-model twin: crx_debug_speculation does not apply)
        crx_kparams_models km = *mdl;
        static_cast<crx_kparams&>(km) = kq;
        return launched(crx_launch_solve_models(km, tmpl, st), "solver (per-problem models)");
    }
    // [r6] The TWO-WAVE instantiation (one obstacle slot, the reference's exponent, N = 12 / 10; crx_kernels.hip SPEC): a second wave per problem factorises
    // with the next entry of the inertia-correction schedule while the first tries the current one.  OPT-IN (crx_debug_speculation), not the default:
    // measured on the headline batch (profiles/r06_speculation.txt) a doomed attempt costs 1.7 us, not a sweep's 5.8 -- the recursion stops at the
    // first non-positive pivot -- so the longest healthy solve (34 iterations, 24 doomed attempts) gains 2.5 % alone and the 256-problem launch, which
    // pays two workgroup barriers per iteration in every problem, loses 1 % (0.4759 -> 0.4805 ms).
    const bool spec = tmpl == 1 && kq.mode == 1 && kq.degree == 6 && (kq.N == 12 || kq.N == 10) && g_spec > 0;
    kq.spec_idle = g_spec == 2;
    return launched(spec ? crx_launch_solve_spec(kq, st) : crx_launch_solve(kq, tmpl, st), "solver");
}

}  // namespace

extern "C" {

int crx_version(void) { return CRX_VERSION; }

const char* crx_last_error(void) { return g_err; }

int crx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int crx_init(int device) {
    std::lock_guard<std::mutex> lk(g_mu);
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(CRX_ERR_NO_DEVICE, "no HIP device visible (%s); libcrx has no CPU back-end",
                    e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(CRX_ERR_ARG, "device %d outside [0,%d)", device, n);
    HIP_TRY(hipSetDevice(device));
    if (g_init && g_device == device) return CRX_OK;
    if (g_init && g_device >= 0) {
        // everything below belongs to the old device: release it there (the trace buffer included)
        (void)hipSetDevice(g_device);
        if (g_stream) { (void)hipStreamDestroy(g_stream); g_stream = nullptr; }
        g_in.release(); g_out.release(); g_hin.release(); g_hout.release(); g_trace.release();
        g_trace_rows = 0;
        HIP_TRY(hipSetDevice(device));
    }
    HIP_TRY(hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking));
    g_device = device;
    g_init = true;
    return CRX_OK;
}

void crx_shutdown(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_init) return;
    (void)hipSetDevice(g_device);
    g_in.release(); g_out.release(); g_hin.release(); g_hout.release(); g_trace.release();
    g_trace_rows = 0;
    if (g_stream) (void)hipStreamDestroy(g_stream);
    g_stream = nullptr;
    g_init = false; g_device = -1;
}

// diagnostics (not in crx.h): record e_d, e_p, e_c, mu, alpha, alpha_dual, delta_w, accept-type per
// iteration of one problem of the following solves
int crx_trace_enable(int problem, int rows) {
    if (int rc = ensure_init()) return rc;
    g_trace_rows = 0;
    const bool sub = rows < 0;   // negative: report Riccati sub-phase cycles in slots 8..11
    if (rows < 0) rows = -rows;
    if (rows == 0) return CRX_OK;
    if (int rc = g_trace.ensure((size_t)rows * 16 * sizeof(double))) return rc;
    HIP_TRY(hipMemset(g_trace.p, 0, (size_t)rows * 16 * sizeof(double)));
    g_trace_rows = sub ? -rows : rows; g_trace_problem = problem;
    return CRX_OK;
}
int crx_trace_read(double* host, int rows) {
    { int cap = g_trace_rows < 0 ? -g_trace_rows : g_trace_rows; if (rows > cap) rows = cap; }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host, g_trace.p, (size_t)rows * 16 * sizeof(double), hipMemcpyDeviceToHost));
    return CRX_OK;
}

// diagnostics (not in crx.h): make the solver kernels fill their LDS slice with NaN before set-up, so that a read
// of LDS the kernel did not write shows up as a changed result (tests/test_gpu_parity.py::test_no_stale_lds_reads)
void crx_debug_poison_lds(int enable) { g_poison = enable != 0; }

// diagnostics (not in crx.h): the solver kernel reports, for every CONVERGED problem of the following planner / CBF solves, an UNSCALED KKT
// quantity of the returned iterate in kkt[] instead of the scaled error -- without IPOPT's s_d = max(100, ||nu||_1 / m) / 100 and with the
// gradient-based row scaling undone (rows in the reference's units).  mode 1: the max of the three; 2: the reduced Lagrangian gradient (IPOPT
// dual_inf); 3: the constraint violation (constr_viol); 4: the complementarity (compl_inf); 0: off.  Since 0.4.0 these are the quantities the
// termination test itself bounds (crx_ipm_opts.dual_inf_tol / constr_viol_tol / compl_inf_tol); bench.py reports each (kkt_unscaled_*_max).
// diagnostics (not in crx.h): the two-wave (speculating) instantiation of the one-obstacle solver kernel -- 0: never (default), 1: whenever it exists
// (A/B runs; tests/test_gpu_parity.py::test_speculating_wave_follows_the_sequential_schedule), 2: that kernel with its second wave left idle (separates
// "another kernel" from "another wave's result" when two runs disagree)
void crx_debug_speculation(int mode) { g_spec = mode < 0 ? 0 : (mode > 2 ? 1 : mode); }

void crx_debug_kkt_unscaled(int mode) { g_kkt_unscaled = (mode >= 0 && mode <= 4) ? mode : 0; }

// diagnostics (not in crx.h): the packed wave reductions and the DPP dot products of crx_wave.h on host data, in [4][64] -> out [16 + 3 * 64]
// (tests/test_gpu_parity.py::test_packed_wave_reductions)
int crx_debug_wave_reduce(const double* in, double* out) {
    if (int rc = ensure_init()) return rc;
    if (!in || !out) return fail(CRX_ERR_ARG, "NULL array argument");
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    Stage sg;
    auto din = sg.in(in, 256);
    auto dout = sg.out(out, 208);
    if (int rc = sg.up(g_stream)) return rc;
    hipError_t e = crx_launch_debug_reduce(sg[din], sg[dout], g_stream);
    if (e != hipSuccess) return fail(CRX_ERR_HIP, "debug reduce launch: %s", hipGetErrorString(e));
    return sg.down(g_stream);
}

// diagnostics (not in crx.h): LDS bytes one problem occupies (= one single-wave workgroup), for the
// "resident problems per CU" figure of bench.py.  kind 0: crx_solve_kernel (N, n_obs_max); 1: crx_lmpc_kernel (N, n_ss_max)
long crx_debug_lds_bytes(int kind, int N, int n) {
    return kind == 0 ? (long)crx_solve_lds_bytes(N, n) : (long)crx_lmpc_lds_bytes(N, n);
}

// diagnostics (not in crx.h): problems resident per CU as the runtime computes it (LDS AND registers); needs a GPU
int crx_debug_resident_per_cu(int kind, int N, int n) {
    if (ensure_init() != CRX_OK) return -1;
    return kind == 0 ? crx_solve_resident_per_cu(N, n) : crx_lmpc_resident_per_cu(N, n);
}

// ---- timers: a pair of HIP events per object, no global state (include/crx.h) -----------------------------------------
struct CrxTimer { hipEvent_t e0, e1; bool armed; };

int crx_timer_create(void** timer) {
    if (int rc = ensure_init()) return rc;
    if (!timer) return fail(CRX_ERR_ARG, "timer is NULL");
    HIP_TRY(hipSetDevice(g_device));
    CrxTimer* t = new CrxTimer{nullptr, nullptr, false};
    if (hipEventCreate(&t->e0) != hipSuccess || hipEventCreate(&t->e1) != hipSuccess) {
        if (t->e0) (void)hipEventDestroy(t->e0);
        delete t;
        return fail(CRX_ERR_HIP, "hipEventCreate failed");
    }
    *timer = t;
    return CRX_OK;
}
int crx_timer_destroy(void* timer) {
    CrxTimer* t = (CrxTimer*)timer;
    if (!t) return CRX_OK;
    (void)hipEventDestroy(t->e0); (void)hipEventDestroy(t->e1);
    delete t;
    return CRX_OK;
}
int crx_timer_begin(void* timer, void* stream) {
    CrxTimer* t = (CrxTimer*)timer;
    if (!t) return fail(CRX_ERR_ARG, "timer is NULL");
    t->armed = false;
    HIP_TRY(hipEventRecord(t->e0, (hipStream_t)stream));
    return CRX_OK;
}
int crx_timer_end(void* timer, void* stream) {
    CrxTimer* t = (CrxTimer*)timer;
    if (!t) return fail(CRX_ERR_ARG, "timer is NULL");
    HIP_TRY(hipEventRecord(t->e1, (hipStream_t)stream));
    t->armed = true;
    return CRX_OK;
}
double crx_timer_ms(void* timer) {
    CrxTimer* t = (CrxTimer*)timer;
    if (!t || !t->armed) return -1.0;
    float ms = 0.f;
    if (hipEventSynchronize(t->e1) != hipSuccess) return -1.0;
    if (hipEventElapsedTime(&ms, t->e0, t->e1) != hipSuccess) return -1.0;
    return (double)ms;
}

void crx_ipm_opts_default(crx_ipm_opts* o) {
    o->tol = 1e-8; o->max_iter = 200; o->restore_iters = 50; o->mu_init = 0.1; o->kappa_eps = 10.0;
    o->kappa_mu = 0.2; o->theta_mu = 1.5; o->tau_min = 0.99; o->slack_push = 1e-2; o->grad_scale_max = 100.0;
    o->reach_screen = 1; o->slack_start = 2;
    o->dual_inf_tol = 1.0; o->constr_viol_tol = 1e-4; o->compl_inf_tol = 1e-4;   // IPOPT's defaults (the reference sets none: control.py:593)
    o->stall_iters = 100; o->qp_method = 0;
}

void crx_planner_desc_default(crx_planner_desc* d, int N, const double* A, const double* B) {
    memset(d, 0, sizeof(*d));
    d->N = N;
    memcpy(d->A, A, sizeof(d->A)); memcpy(d->B, B, sizeof(d->B));
    d->w_ref = 20.0; d->w_dey = 30.0; d->w_prog = 200.0; d->vx_max = 5.0; d->delta_max = 0.5; d->a_max = 1.5;
    d->dt_ref = 0.1; d->fallback_gain = 1.1;
    crx_ipm_opts_default(&d->opts);
}

void crx_cbf_desc_default(crx_cbf_desc* d, int N, int n_obs_max, const double* A, const double* B) {
    memset(d, 0, sizeof(*d));
    d->N = N; d->n_obs_max = n_obs_max; d->per_stage_target = 0; d->degree = 6;
    memcpy(d->A, A, sizeof(d->A)); memcpy(d->B, B, sizeof(d->B));
    const double Q[6] = {10.0, 0.0, 0.0, 4.0, 0.0, 40.0};
    memcpy(d->Q, Q, sizeof(Q)); d->R[0] = 0.1; d->R[1] = 0.1;
    d->delta_max = 0.5; d->a_max = 1.0; d->v_min = 0.0; d->v_max = 10.0; d->ey_max = 1.0;
    d->alpha = 0.8; d->margin = 0.2; d->l_sum = 0.4; d->w_sum = 0.2; d->w_slack = 1e4;
    crx_ipm_opts_default(&d->opts);
    // budgets by problem class (include/crx.h crx_ipm_opts.stall_iters): the short one-obstacle class is done after 30 iterations when
    // healthy, the three-obstacle N = 20 class needs 53..86
    if (N <= 12 && n_obs_max <= 1) { d->opts.stall_iters = 50; d->opts.restore_iters = 25; }
}

void crx_select_desc_default(crx_select_desc* d, int N, int n_veh_max, double lap_length) {
    d->N = N; d->n_veh_max = n_veh_max; d->veh_length = 0.4; d->veh_width = 0.2; d->lap_length = lap_length;
    d->w_prog = 10.0; d->w_coll = 100.0; d->w_switch = 100.0;
}

// ---- planner --------------------------------------------------------------------------------------
// Every family below has ONE statement of what its host-pointer and its _dev entry points refuse alike: the descriptor, the
// dimensions and the NULL-pointer list (not looked at by an empty call, which succeeds).  The host-pointer entry point adds the
// per-element checks on host arrays and calls the _dev entry point on the staged copies.
static bool planner_null(arr x0, arr bez_s, arr bez_ey, arr ey_lb, arr ey_ub, arr X, arr U, arr cost, arr status, arr kkt, arr iters) {
    return any_null(x0, bez_s, bez_ey, ey_lb, ey_ub, X, U, cost, status, kkt, iters);
}

// (own_model = false: one model per problem is given, d->A and d->B are not read)
static int check_planner(crx_kparams& kp, const crx_planner_desc* d, int batch, bool own_model, arr x0, arr bez_s, arr bez_ey, arr ey_lb, arr ey_ub,
                         arr X, arr U, arr cost, arr status, arr kkt, arr iters) {
    if (int rc = ensure_init()) return rc;
    if (int rc = fill_planner(kp, d, batch, own_model)) return rc;
    if (batch > 0 && planner_null(x0, bez_s, bez_ey, ey_lb, ey_ub, X, U, cost, status, kkt, iters))
        return fail(CRX_ERR_ARG, "NULL array argument");
    return 0;
}

// the one thing the models entry points refuse on top of check_planner: every model array, or none (n_given of n_all).  Pointers only, so it is
// looked at before the device is
static int check_planner_models(int n_given, int n_all) {
    if (n_given != 0 && n_given != n_all)
        return fail(CRX_ERR_ARG, n_all == 3 ? "model_A, model_B and model_reach go together: all three or none (%d of 3 given)"
                                            : "model_A and model_B go together: both or neither (%d of 2 given)", n_given);
    return 0;
}

// every planner launch: active_div problems share one entry of active (the regions of a scenario; 0: one each); models all three or none
static int planner_solve_masked(const crx_planner_desc* d, int batch, const int32_t* active, int active_div, const double* x0,
                                const double* model_A, const double* model_B, const double* model_reach, const double* bez_s,
                                const double* bez_ey, const double* ey_lb, const double* ey_ub, double* X, double* U, double* cost,
                                int32_t* status, double* kkt, int32_t* iters, void* stream) {
    crx_kparams_models km;
    crx_kparams& kp = km;
    if (int rc = check_planner_models((model_A != nullptr) + (model_B != nullptr) + (model_reach != nullptr), 3)) return rc;
    if (int rc = check_planner(kp, d, batch, !model_A, x0, bez_s, bez_ey, ey_lb, ey_ub, X, U, cost, status, kkt, iters)) return rc;
    if (batch == 0) return CRX_OK;
    kp.x0 = x0; kp.bez_s = bez_s; kp.bez_ey = bez_ey; kp.ey_lb = ey_lb; kp.ey_ub = ey_ub;
    kp.X = X; kp.U = U; kp.sigma = nullptr; kp.cost = cost; kp.status = status; kp.kkt = kkt; kp.iters = iters;
    kp.active = active; kp.active_div = active_div;
    km.model_A = model_A; km.model_B = model_B; km.model_reach = model_reach;
    return launch_solve(kp, 0, (hipStream_t)stream, model_A ? &km : nullptr);
}

int crx_planner_solve_dev(const crx_planner_desc* d, int batch, const double* x0, const double* bez_s,
                          const double* bez_ey, const double* ey_lb, const double* ey_ub, double* X, double* U,
                          double* cost, int32_t* status, double* kkt, int32_t* iters, void* stream) {
    return crx_planner_solve_models_dev(d, batch, nullptr, x0, nullptr, nullptr, nullptr, bez_s, bez_ey, ey_lb, ey_ub, X, U, cost, status, kkt, iters,
                                        stream);
}

int crx_planner_solve_models_dev(const crx_planner_desc* d, int batch, const int32_t* active, const double* x0, const double* model_A,
                                 const double* model_B, const double* model_reach, const double* bez_s, const double* bez_ey,
                                 const double* ey_lb, const double* ey_ub, double* X, double* U, double* cost, int32_t* status, double* kkt,
                                 int32_t* iters, void* stream) {
    return planner_solve_masked(d, batch, active, 0, x0, model_A, model_B, model_reach, bez_s, bez_ey, ey_lb, ey_ub, X, U, cost, status, kkt, iters,
                                stream);
}

int crx_planner_models_reach_dev(const crx_planner_desc* d, int batch, const double* model_A, const double* model_B, double* model_reach,
                                 void* stream) {
    if (int rc = ensure_init()) return rc;
    crx_kparams kp;
    if (int rc = fill_planner(kp, d, batch, false)) return rc;
    if (batch == 0) return CRX_OK;
    if (any_null(model_A, model_B, model_reach)) return fail(CRX_ERR_ARG, "NULL array argument");
    return launched(crx_launch_planner_reach(d->N, batch, d->delta_max, d->a_max, model_A, model_B, model_reach, (hipStream_t)stream), "planner reach");
}

int crx_planner_solve(const crx_planner_desc* d, int batch, const double* x0, const double* bez_s,
                      const double* bez_ey, const double* ey_lb, const double* ey_ub, double* X, double* U,
                      double* cost, int32_t* status, double* kkt, int32_t* iters) {
    return crx_planner_solve_models(d, batch, x0, nullptr, nullptr, bez_s, bez_ey, ey_lb, ey_ub, X, U, cost, status, kkt, iters);
}

// (non-finite model entries are no argument error: that problem reports CRX_SINGULAR with the fall-back trajectory, as on the device path)
int crx_planner_solve_models(const crx_planner_desc* d, int batch, const double* x0, const double* model_A, const double* model_B,
                             const double* bez_s, const double* bez_ey, const double* ey_lb, const double* ey_ub, double* X, double* U,
                             double* cost, int32_t* status, double* kkt, int32_t* iters) {
    crx_kparams chk;
    const bool models = model_A || model_B;
    if (int rc = check_planner_models((model_A != nullptr) + (model_B != nullptr), 2)) return rc;
    if (int rc = check_planner(chk, d, batch, !models, x0, bez_s, bez_ey, ey_lb, ey_ub, X, U, cost, status, kkt, iters)) return rc;
    if (batch == 0) return CRX_OK;
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    const size_t B = (size_t)batch, N = (size_t)d->N;
    Stage sg;
    auto dx0 = sg.in(x0, B * 6); auto dbs = sg.in(bez_s, B * (N + 1)); auto dbe = sg.in(bez_ey, B * (N + 1));
    auto dlb = sg.in(ey_lb, B * N); auto dub = sg.in(ey_ub, B);
    auto dmA = models ? sg.in(model_A, B * 36) : Stage::Ref<double>{};
    auto dmB = models ? sg.in(model_B, B * 12) : Stage::Ref<double>{};
    auto dmR = models ? sg.scratch(CRX_PLANNER_MODEL_REACH_DOUBLES(B) * sizeof(double)) : Stage::Ref<char>{};
    auto dX = sg.out(X, B * (N + 1) * 6); auto dU = sg.out(U, B * N * 2); auto dc = sg.out(cost, B);
    auto dk = sg.out(kkt, B); auto ds = sg.out(status, B); auto di = sg.out(iters, B);
    if (int rc = sg.up(g_stream)) return rc;
    if (models)
        if (int rc = crx_planner_models_reach_dev(d, batch, sg[dmA], sg[dmB], (double*)sg[dmR], g_stream)) return rc;
    if (int rc = crx_planner_solve_models_dev(d, batch, nullptr, sg[dx0], sg[dmA], sg[dmB], (double*)sg[dmR], sg[dbs], sg[dbe], sg[dlb], sg[dub],
                                              sg[dX], sg[dU], sg[dc], sg[ds], sg[dk], sg[di], g_stream)) return rc;
    return sg.down(g_stream);
}

// ---- MPC-CBF ---------------------------------------------------------------------------------------
int crx_cbf_solve_dev(const crx_cbf_desc* d, int batch, const double* x0, const double* xt, const double* obs_s,
                      const double* obs_ey, const double* lap_off, const int32_t* n_obs, double* X, double* U,
                      double* sigma, double* cost, int32_t* status, double* kkt, int32_t* iters, void* stream) {
    return crx_cbf_solve_masked_dev(d, batch, nullptr, x0, xt, obs_s, obs_ey, lap_off, n_obs, X, U, sigma, cost, status, kkt, iters, stream);
}

int crx_cbf_solve_masked_dev(const crx_cbf_desc* d, int batch, const int32_t* active, const double* x0, const double* xt,
                             const double* obs_s, const double* obs_ey, const double* lap_off, const int32_t* n_obs, double* X,
                             double* U, double* sigma, double* cost, int32_t* status, double* kkt, int32_t* iters, void* stream) {
    return crx_cbf_solve_ordered_dev(d, batch, active, nullptr, x0, xt, obs_s, obs_ey, lap_off, n_obs, nullptr, X, U, sigma, cost, status, kkt, iters, stream);
}

int crx_cbf_solve_dims_dev(const crx_cbf_desc* d, int batch, const int32_t* active, const double* x0, const double* xt,
                           const double* obs_s, const double* obs_ey, const double* lap_off, const int32_t* n_obs,
                           const double* obs_dims, double* X, double* U, double* sigma, double* cost, int32_t* status, double* kkt,
                           int32_t* iters, void* stream) {
    return crx_cbf_solve_ordered_dev(d, batch, active, nullptr, x0, xt, obs_s, obs_ey, lap_off, n_obs, obs_dims, X, U, sigma, cost, status, kkt, iters, stream);
}

static int check_cbf(crx_kparams& kp, const crx_cbf_desc* d, int batch, arr x0, arr xt, arr obs_s, arr obs_ey, arr lap_off, arr n_obs, arr X, arr U,
                     arr sigma, arr cost, arr status, arr kkt, arr iters) {
    if (int rc = ensure_init()) return rc;
    if (int rc = fill_cbf(kp, d, batch)) return rc;
    if (batch == 0) return 0;
    if (any_null(x0, xt, X, U, cost, status, kkt, iters)) return fail(CRX_ERR_ARG, "NULL array argument");
    if (d->n_obs_max > 0 && any_null(obs_s, obs_ey, lap_off, n_obs, sigma))
        return fail(CRX_ERR_ARG, "NULL obstacle array with n_obs_max > 0");
    return 0;
}

int crx_cbf_solve_ordered_dev(const crx_cbf_desc* d, int batch, const int32_t* active, const int32_t* order, const double* x0,
                              const double* xt, const double* obs_s, const double* obs_ey, const double* lap_off,
                              const int32_t* n_obs, const double* obs_dims, double* X, double* U, double* sigma, double* cost,
                              int32_t* status, double* kkt, int32_t* iters, void* stream) {
    return crx_cbf_solve_models_dev(d, batch, active, order, x0, nullptr, nullptr, nullptr, xt, obs_s, obs_ey, lap_off, n_obs, obs_dims, X, U, sigma,
                                    cost, status, kkt, iters, stream);
}

// the one thing the models entry points refuse on top of check_cbf: all three model arrays, or none
static int check_cbf_models(arr model_A, arr model_B, arr model_reach) {
    const int n = (model_A != nullptr) + (model_B != nullptr) + (model_reach != nullptr);
    if (n != 0 && n != 3) return fail(CRX_ERR_ARG, "model_A, model_B and model_reach go together: all three or none (%d of 3 given)", n);
    return 0;
}

int crx_cbf_solve_models_dev(const crx_cbf_desc* d, int batch, const int32_t* active, const int32_t* order, const double* x0,
                             const double* model_A, const double* model_B, const double* model_reach, const double* xt,
                             const double* obs_s, const double* obs_ey, const double* lap_off, const int32_t* n_obs,
                             const double* obs_dims, double* X, double* U, double* sigma, double* cost, int32_t* status, double* kkt,
                             int32_t* iters, void* stream) {
    crx_kparams_models km;
    crx_kparams& kp = km;
    if (int rc = check_cbf(kp, d, batch, x0, xt, obs_s, obs_ey, lap_off, n_obs, X, U, sigma, cost, status, kkt, iters)) return rc;
    if (int rc = check_cbf_models(model_A, model_B, model_reach)) return rc;
    if (batch == 0) return CRX_OK;
    kp.x0 = x0; kp.xt = xt; kp.obs_s = obs_s; kp.obs_ey = obs_ey; kp.lap_off = lap_off; kp.n_obs = n_obs;
    kp.X = X; kp.U = U; kp.sigma = sigma; kp.cost = cost; kp.status = status; kp.kkt = kkt; kp.iters = iters;
    kp.active = active; kp.order = order; kp.obs_dims = d->n_obs_max > 0 ? obs_dims : nullptr;
    km.model_A = model_A; km.model_B = model_B; km.model_reach = model_reach;
    return launch_solve(kp, d->n_obs_max, (hipStream_t)stream, model_A ? &km : nullptr);
}

int crx_cbf_models_reach_dev(const crx_cbf_desc* d, int batch, const double* model_A, const double* model_B, double* model_reach, void* stream) {
    if (int rc = ensure_init()) return rc;
    crx_kparams kp;
    if (int rc = fill_cbf(kp, d, batch)) return rc;
    if (batch == 0) return CRX_OK;
    if (any_null(model_A, model_B, model_reach)) return fail(CRX_ERR_ARG, "NULL array argument");
    return launched(crx_launch_cbf_reach(d->N, batch, d->delta_max, d->a_max, model_A, model_B, model_reach, (hipStream_t)stream), "cbf reach");
}

int crx_cbf_solve(const crx_cbf_desc* d, int batch, const double* x0, const double* xt, const double* obs_s,
                  const double* obs_ey, const double* lap_off, const int32_t* n_obs, double* X, double* U,
                  double* sigma, double* cost, int32_t* status, double* kkt, int32_t* iters) {
    return crx_cbf_solve_dims(d, batch, x0, xt, obs_s, obs_ey, lap_off, n_obs, nullptr, X, U, sigma, cost, status, kkt, iters);
}

int crx_cbf_solve_dims(const crx_cbf_desc* d, int batch, const double* x0, const double* xt, const double* obs_s,
                  const double* obs_ey, const double* lap_off, const int32_t* n_obs, const double* obs_dims, double* X, double* U,
                  double* sigma, double* cost, int32_t* status, double* kkt, int32_t* iters) {
    return crx_cbf_solve_models(d, batch, x0, nullptr, nullptr, xt, obs_s, obs_ey, lap_off, n_obs, obs_dims, X, U, sigma, cost, status, kkt, iters);
}

// (non-finite model entries are no argument error: that problem reports CRX_SINGULAR, as on the device path)
int crx_cbf_solve_models(const crx_cbf_desc* d, int batch, const double* x0, const double* model_A, const double* model_B, const double* xt,
                         const double* obs_s, const double* obs_ey, const double* lap_off, const int32_t* n_obs, const double* obs_dims,
                         double* X, double* U, double* sigma, double* cost, int32_t* status, double* kkt, int32_t* iters) {
    crx_kparams chk;
    if (int rc = check_cbf(chk, d, batch, x0, xt, obs_s, obs_ey, lap_off, n_obs, X, U, sigma, cost, status, kkt, iters)) return rc;
    const bool models = model_A || model_B;
    if (!model_A != !model_B) return fail(CRX_ERR_ARG, "model_A and model_B go together: both or neither (%s is NULL)", model_A ? "model_B" : "model_A");
    if (batch == 0) return CRX_OK;
    const size_t B = (size_t)batch, N = (size_t)d->N, V = (size_t)d->n_obs_max;
    if (V > 0) {
        for (size_t b = 0; b < B; b++)
            if (n_obs[b] < 0 || n_obs[b] > (int)V) return fail(CRX_ERR_ARG, "n_obs[%zu]=%d outside [0,%zu]", b, n_obs[b], V);
        if (obs_dims)
            for (size_t b = 0; b < B; b++)
                for (int o = 0; o < n_obs[b]; o++)
                    if (!(obs_dims[(b * V + o) * 2] > 0.0) || !(obs_dims[(b * V + o) * 2 + 1] > 0.0))
                        return fail(CRX_ERR_ARG, "obs_dims[%zu][%d] must be positive", b, o);
    }
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    const size_t n_ob = B * V * (N + 1);
    Stage sg;
    auto dx0 = sg.in(x0, B * 6); auto dxt = sg.in(xt, d->per_stage_target ? B * (N + 1) * 6 : B * 6);
    auto dos = sg.in(obs_s, n_ob); auto doe = sg.in(obs_ey, n_ob); auto dlo = sg.in(lap_off, B * V);
    auto ddm = (obs_dims && V > 0) ? sg.in(obs_dims, B * V * 2) : Stage::Ref<double>{};
    auto dno = sg.in(V > 0 ? n_obs : (const int32_t*)nullptr, B);
    auto dmA = models ? sg.in(model_A, B * 36) : Stage::Ref<double>{};
    auto dmB = models ? sg.in(model_B, B * 12) : Stage::Ref<double>{};
    auto dmR = models ? sg.scratch(CRX_CBF_MODEL_REACH_DOUBLES(B) * sizeof(double)) : Stage::Ref<char>{};
    auto dX = sg.out(X, B * (N + 1) * 6); auto dU = sg.out(U, B * N * 2); auto dsg = sg.out(sigma, n_ob);
    auto dc = sg.out(cost, B); auto dk = sg.out(kkt, B); auto ds = sg.out(status, B); auto di = sg.out(iters, B);
    if (int rc = sg.up(g_stream)) return rc;
    if (models)
        if (int rc = crx_cbf_models_reach_dev(d, batch, sg[dmA], sg[dmB], (double*)sg[dmR], g_stream)) return rc;
    if (int rc = crx_cbf_solve_models_dev(d, batch, nullptr, nullptr, sg[dx0], sg[dmA], sg[dmB], (double*)sg[dmR], sg[dxt], sg[dos], sg[doe],
                                          sg[dlo], sg[dno], sg[ddm], sg[dX], sg[dU], sg[dsg], sg[dc], sg[ds], sg[dk], sg[di], g_stream)) return rc;
    return sg.down(g_stream);
}

// ---- selection -------------------------------------------------------------------------------------
static int check_select(const crx_select_desc* d, int n_scen) {
    if (!d) return fail(CRX_ERR_ARG, "desc is NULL");
    if (d->N < 1 || d->N > CRX_MAX_N || d->n_veh_max < 0 || d->n_veh_max > CRX_MAX_VEH || n_scen < 0)
        return fail(CRX_ERR_ARG, "bad selection dimensions");
    // the kernel wraps predicted s by lap_length (overtake_traj_planner.py:216-217): a zeroed descriptor must be a call
    // failure, not a device loop
    if (!(d->lap_length > 0.0) || !isfinite(d->lap_length)) return fail(CRX_ERR_ARG, "lap_length must be positive and finite");
    if (!(d->veh_length >= 0.0) || !(d->veh_width >= 0.0)) return fail(CRX_ERR_ARG, "vehicle dimensions must be non-negative");
    return 0;
}

static bool select_null(const crx_select_desc* d, arr n_veh, arr X, arr obs_s, arr obs_ey, arr old_flag, arr flag, arr sel_cost, arr best_X) {
    return any_null(n_veh, X, old_flag, flag, sel_cost, best_X) || (d->n_veh_max > 0 && any_null(obs_s, obs_ey));
}

static int check_select_call(const crx_select_desc* d, int n_scen, arr n_veh, arr X, arr obs_s, arr obs_ey, arr old_flag, arr flag, arr sel_cost,
                             arr best_X) {
    if (int rc = ensure_init()) return rc;
    if (int rc = check_select(d, n_scen)) return rc;
    if (n_scen > 0 && select_null(d, n_veh, X, obs_s, obs_ey, old_flag, flag, sel_cost, best_X)) return fail(CRX_ERR_ARG, "NULL array argument");
    return 0;
}

int crx_select_dev(const crx_select_desc* d, int n_scen, const int32_t* n_veh, const double* X, const double* obs_s,
                   const double* obs_ey, const int32_t* old_flag, int32_t* flag, double* sel_cost, double* best_X,
                   void* stream) {
    if (int rc = check_select_call(d, n_scen, n_veh, X, obs_s, obs_ey, old_flag, flag, sel_cost, best_X)) return rc;
    if (n_scen == 0) return CRX_OK;
    crx_select_kparams sp;
    sp.N = d->N; sp.V = d->n_veh_max; sp.n_scen = n_scen;
    sp.veh_length = d->veh_length; sp.veh_width = d->veh_width; sp.lap_length = d->lap_length;
    sp.w_prog = d->w_prog; sp.w_coll = d->w_coll; sp.w_switch = d->w_switch;
    sp.n_veh = n_veh; sp.X = X; sp.obs_s = obs_s; sp.obs_ey = obs_ey; sp.old_flag = old_flag;
    sp.flag = flag; sp.sel_cost = sel_cost; sp.best_X = best_X;
    return launched(crx_launch_select(sp, (hipStream_t)stream), "selection");
}

int crx_select(const crx_select_desc* d, int n_scen, const int32_t* n_veh, const double* X, const double* obs_s,
               const double* obs_ey, const int32_t* old_flag, int32_t* flag, double* sel_cost, double* best_X) {
    if (int rc = check_select_call(d, n_scen, n_veh, X, obs_s, obs_ey, old_flag, flag, sel_cost, best_X)) return rc;
    if (n_scen == 0) return CRX_OK;
    const size_t S = (size_t)n_scen, N = (size_t)d->N, V = (size_t)d->n_veh_max, R = V + 1;
    for (size_t s = 0; s < S; s++)
        if (n_veh[s] < 0 || n_veh[s] > (int)V) return fail(CRX_ERR_ARG, "n_veh[%zu]=%d outside [0,%zu]", s, n_veh[s], V);
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    Stage sg;
    auto dX = sg.in(X, S * R * (N + 1) * 6); auto dos = sg.in(obs_s, S * V * (N + 1)); auto doe = sg.in(obs_ey, S * V * (N + 1));
    auto dnv = sg.in(n_veh, S); auto dof = sg.in(old_flag, S);
    auto dfl = sg.out(flag, S); auto dsc = sg.out(sel_cost, S * R); auto dbX = sg.out(best_X, S * (N + 1) * 6);
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_select_dev(d, n_scen, sg[dnv], sg[dX], sg[dos], sg[doe], sg[dof], sg[dfl], sg[dsc], sg[dbX], g_stream)) return rc;
    return sg.down(g_stream);
}

// ---- overtake path planner QP -----------------------------------------------------------------------
void crx_path_desc_default(crx_path_desc* d, int N, double alpha) {
    memset(d, 0, sizeof(*d));
    d->N = N; d->alpha = alpha; d->w_rate = 100.0;
    crx_ipm_opts_default(&d->opts);
}

static int fill_path(crx_path_kparams& pp, const crx_path_desc* d, int batch) {
    if (!d) return fail(CRX_ERR_ARG, "desc is NULL");
    if (d->N < 2 || d->N > CRX_MAX_N) return fail(CRX_ERR_ARG, "N=%d outside [2,%d]", d->N, CRX_MAX_N);
    if (!(d->alpha >= 0.0 && d->alpha <= 1.0) || !(d->w_rate >= 0.0)) return fail(CRX_ERR_ARG, "alpha outside [0,1] or w_rate < 0");
    if (batch < 0) return fail(CRX_ERR_ARG, "batch < 0");
    if (int rc = check_opts(d->opts)) return rc;
    memset(&pp, 0, sizeof(pp));
    pp.N = d->N; pp.batch = batch; pp.alpha = d->alpha; pp.w_rate = d->w_rate; pp.opts = d->opts;
    return 0;
}

static int check_path(crx_path_kparams& pp, const crx_path_desc* d, int batch, arr opt, arr bez, arr lb, arr ub, arr e0, arr eN, arr E, arr cost,
                      arr status, arr kkt, arr iters) {
    if (int rc = ensure_init()) return rc;
    if (int rc = fill_path(pp, d, batch)) return rc;
    if (batch > 0 && any_null(opt, bez, lb, ub, e0, eN, E, cost, status, kkt, iters)) return fail(CRX_ERR_ARG, "NULL array argument");
    return 0;
}

int crx_path_solve_dev(const crx_path_desc* d, int batch, const double* opt, const double* bez, const double* lb,
                       const double* ub, const double* e0, const double* eN, double* E, double* cost, int32_t* status,
                       double* kkt, int32_t* iters, void* stream) {
    crx_path_kparams pp;
    if (int rc = check_path(pp, d, batch, opt, bez, lb, ub, e0, eN, E, cost, status, kkt, iters)) return rc;
    if (batch == 0) return CRX_OK;
    pp.opt = opt; pp.bez = bez; pp.lb = lb; pp.ub = ub; pp.e0 = e0; pp.eN = eN;
    pp.E = E; pp.cost = cost; pp.status = status; pp.kkt = kkt; pp.iters = iters;
    return launched(crx_launch_path(pp, (hipStream_t)stream), "path");
}

int crx_path_solve(const crx_path_desc* d, int batch, const double* opt, const double* bez, const double* lb,
                   const double* ub, const double* e0, const double* eN, double* E, double* cost, int32_t* status,
                   double* kkt, int32_t* iters) {
    crx_path_kparams chk;
    if (int rc = check_path(chk, d, batch, opt, bez, lb, ub, e0, eN, E, cost, status, kkt, iters)) return rc;
    if (batch == 0) return CRX_OK;
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    const size_t B = (size_t)batch, n1 = B * (size_t)(d->N + 1);
    Stage sg;
    auto dop = sg.in(opt, n1); auto dbz = sg.in(bez, n1); auto dlb = sg.in(lb, n1); auto dub = sg.in(ub, n1);
    auto d0 = sg.in(e0, B); auto dN = sg.in(eN, B);
    auto dE = sg.out(E, n1); auto dc = sg.out(cost, B); auto dk = sg.out(kkt, B); auto ds = sg.out(status, B); auto di = sg.out(iters, B);
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_path_solve_dev(d, batch, sg[dop], sg[dbz], sg[dlb], sg[dub], sg[d0], sg[dN], sg[dE], sg[dc], sg[ds], sg[dk], sg[di],
                                    g_stream)) return rc;
    return sg.down(g_stream);
}

// ---- overtake path planner around its QPs (crx_pathplan.hip) ------------------------------------------
void crx_pathprep_desc_default(crx_pathprep_desc* d, int N, int n_veh_max, int n_all_max, int n_opt, double track_width, double lap_length) {
    memset(d, 0, sizeof(*d));
    d->N = N; d->n_veh_max = n_veh_max; d->n_opt = n_opt; d->n_all_max = n_all_max;
    d->safety_factor = 4.5; d->prediction_factor = 0.5; d->lookahead = 4.0; d->next_lap_range = 20.0;
    d->track_width = track_width; d->lap_length = lap_length; d->veh_length = 0.4; d->veh_width = 0.2; d->a_max_plan = 1.5;
}

// the family's one check.  The arguments are looked at BEFORE the library's state: a refusal needs no device.  qd / plan: the fused step
static int check_pathplan(crx_pathplan_kparams& pp, const crx_pathprep_desc* d, const crx_path_desc* qd, bool plan, int n_scen, arr x_wrapped,
                          arr x_raw, arr n_veh, arr order, arr veh_xcurv, arr max_dv, arr obs_ey, arr opt_s, arr opt_ey, arr opt_vx, arr opt, arr bez,
                          arr lb, arr ub, arr e0, arr eN, arr span, arr qp_active, arr E, arr cost, arr status, arr kkt, arr iters, arr flag,
                          arr target, arr plan_status) {
    if (!d) return fail(CRX_ERR_ARG, "desc is NULL");
    if (d->N < 2 || d->N > CRX_MAX_N) return fail(CRX_ERR_ARG, "N=%d outside [2,%d]", d->N, CRX_MAX_N);
    if (d->n_veh_max < 1 || d->n_veh_max > CRX_MAX_VEH) return fail(CRX_ERR_ARG, "n_veh_max=%d outside [1,%d]", d->n_veh_max, CRX_MAX_VEH);
    if (d->n_all_max < 1) return fail(CRX_ERR_ARG, "n_all_max < 1");
    if (d->n_opt < 2) return fail(CRX_ERR_ARG, "n_opt < 2");
    if (n_scen < 0) return fail(CRX_ERR_ARG, "n_scen < 0");
    if (!(d->lap_length > 0.0) || !(d->track_width > 0.0)) return fail(CRX_ERR_ARG, "lap_length and track_width must be positive");
    if (plan) {
        crx_path_kparams qp;
        if (int rc = fill_path(qp, qd, n_scen)) return rc;
        if (qd->N != d->N) return fail(CRX_ERR_ARG, "the two descriptors disagree on N (%d, %d)", d->N, qd->N);
    }
    if (n_scen > 0 && any_null(x_wrapped, x_raw, n_veh, order, veh_xcurv, max_dv, obs_ey, opt_s, opt_ey, opt, bez, lb, ub, e0, eN, span))
        return fail(CRX_ERR_ARG, "NULL array argument");
    if (n_scen > 0 && plan && any_null(opt_vx, qp_active, E, cost, status, kkt, iters, flag, target, plan_status))
        return fail(CRX_ERR_ARG, "NULL array argument");
    if (int rc = ensure_init()) return rc;
    memset(&pp, 0, sizeof(pp));
    pp.d = *d; pp.n_scen = n_scen;
    return 0;
}

int crx_path_prep_dev(const crx_pathprep_desc* d, int n_scen, const double* x_wrapped, const double* x_raw, const int32_t* n_veh,
                      const int32_t* order, const double* veh_xcurv, const double* max_dv, const double* obs_ey, const double* opt_s,
                      const double* opt_ey, double* opt, double* bez, double* lb, double* ub, double* e0, double* eN, double* span,
                      void* stream) {
    crx_pathplan_kparams pp;
    if (int rc = check_pathplan(pp, d, nullptr, false, n_scen, x_wrapped, x_raw, n_veh, order, veh_xcurv, max_dv, obs_ey, opt_s, opt_ey, nullptr,
                                opt, bez, lb, ub, e0, eN, span, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))
        return rc;
    if (n_scen == 0) return CRX_OK;
    pp.x_wrapped = x_wrapped; pp.x_raw = x_raw; pp.n_veh = n_veh; pp.order = order; pp.veh_xcurv = veh_xcurv; pp.max_dv = max_dv;
    pp.obs_ey = obs_ey; pp.opt_s = opt_s; pp.opt_ey = opt_ey;
    pp.opt = opt; pp.bez = bez; pp.lb = lb; pp.ub = ub; pp.e0 = e0; pp.eN = eN; pp.span = span;
    return launched(crx_launch_pathprep(pp, (hipStream_t)stream), "pathprep");
}

int crx_path_plan_dev(const crx_pathprep_desc* d, const crx_path_desc* qd, int n_scen, const int32_t* active, const double* x_wrapped,
                      const double* x_raw, const int32_t* n_veh, const int32_t* order, const double* veh_xcurv, const double* max_dv,
                      const double* obs_ey, const double* opt_s, const double* opt_ey, const double* opt_vx, double* opt, double* bez,
                      double* lb, double* ub, double* e0, double* eN, double* span, int32_t* qp_active, double* E, double* cost,
                      int32_t* status, double* kkt, int32_t* iters, int32_t* flag, double* target, int32_t* plan_status, void* stream) {
    crx_pathplan_kparams pp;
    if (int rc = check_pathplan(pp, d, qd, true, n_scen, x_wrapped, x_raw, n_veh, order, veh_xcurv, max_dv, obs_ey, opt_s, opt_ey, opt_vx, opt,
                                bez, lb, ub, e0, eN, span, qp_active, E, cost, status, kkt, iters, flag, target, plan_status))
        return rc;
    if (n_scen == 0) return CRX_OK;
    pp.x_wrapped = x_wrapped; pp.x_raw = x_raw; pp.n_veh = n_veh; pp.order = order; pp.veh_xcurv = veh_xcurv; pp.max_dv = max_dv;
    pp.obs_ey = obs_ey; pp.opt_s = opt_s; pp.opt_ey = opt_ey; pp.opt_vx = opt_vx; pp.active = active;
    pp.opt = opt; pp.bez = bez; pp.lb = lb; pp.ub = ub; pp.e0 = e0; pp.eN = eN; pp.span = span; pp.qp_active = qp_active;
    pp.E = E; pp.cost = cost; pp.flag = flag; pp.target = target; pp.plan_status = plan_status;
    crx_path_kparams_masked qp;
    const int batch = n_scen * (d->n_veh_max + 1);
    if (int rc = fill_path(qp, qd, batch)) return rc;
    qp.opt = opt; qp.bez = bez; qp.lb = lb; qp.ub = ub; qp.e0 = e0; qp.eN = eN;
    qp.E = E; qp.cost = cost; qp.status = status; qp.kkt = kkt; qp.iters = iters; qp.active = qp_active;
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = launched(crx_launch_pathprep(pp, st), "pathprep")) return rc;
    if (int rc = launched(crx_launch_path_masked(qp, st), "path (masked)")) return rc;
    return launched(crx_launch_pathselect(pp, st), "pathselect");
}

// host-pointer n_veh / order can be validated (the device entries clamp)
static int check_pathplan_host(const crx_pathprep_desc* d, int n_scen, const int32_t* n_veh, const int32_t* order) {
    for (int i = 0; i < n_scen; i++) {
        if (n_veh[i] < 0 || n_veh[i] > d->n_veh_max) return fail(CRX_ERR_ARG, "n_veh[%d]=%d outside [0,%d]", i, n_veh[i], d->n_veh_max);
        for (int k = 0; k < n_veh[i]; k++) {
            const int v = order[(size_t)i * d->n_veh_max + k];
            if (v < 0 || v >= d->n_all_max) return fail(CRX_ERR_ARG, "order[%d][%d]=%d outside [0,%d)", i, k, v, d->n_all_max);
        }
    }
    return 0;
}

int crx_path_prep(const crx_pathprep_desc* d, int n_scen, const double* x_wrapped, const double* x_raw, const int32_t* n_veh,
                  const int32_t* order, const double* veh_xcurv, const double* max_dv, const double* obs_ey, const double* opt_s,
                  const double* opt_ey, double* opt, double* bez, double* lb, double* ub, double* e0, double* eN, double* span) {
    crx_pathplan_kparams chk;
    if (int rc = check_pathplan(chk, d, nullptr, false, n_scen, x_wrapped, x_raw, n_veh, order, veh_xcurv, max_dv, obs_ey, opt_s, opt_ey, nullptr,
                                opt, bez, lb, ub, e0, eN, span, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))
        return rc;
    if (n_scen == 0) return CRX_OK;
    if (int rc = check_pathplan_host(d, n_scen, n_veh, order)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    const size_t S = (size_t)n_scen, N1 = (size_t)d->N + 1, V = (size_t)d->n_veh_max, R = V + 1, T = (size_t)d->n_opt;
    Stage sg;
    auto dxw = sg.in(x_wrapped, S * 6); auto dxr = sg.in(x_raw, S * 6); auto dnv = sg.in(n_veh, S); auto dor = sg.in(order, S * V);
    auto dvx = sg.in(veh_xcurv, S * (size_t)d->n_all_max * 6); auto dmd = sg.in(max_dv, S); auto doe = sg.in(obs_ey, S * V * N1);
    auto dts = sg.in(opt_s, T); auto dte = sg.in(opt_ey, T);
    // in/out: a scenario without vehicles keeps what the caller's arrays held
    auto dop = sg.inout(opt, S * R * N1); auto dbz = sg.inout(bez, S * R * N1); auto dlb = sg.inout(lb, S * R * N1);
    auto dub = sg.inout(ub, S * R * N1); auto d0 = sg.inout(e0, S * R); auto dN = sg.inout(eN, S * R); auto dsp = sg.inout(span, S);
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_path_prep_dev(d, n_scen, sg[dxw], sg[dxr], sg[dnv], sg[dor], sg[dvx], sg[dmd], sg[doe], sg[dts], sg[dte], sg[dop], sg[dbz],
                                   sg[dlb], sg[dub], sg[d0], sg[dN], sg[dsp], g_stream)) return rc;
    return sg.down(g_stream);
}

int crx_path_plan(const crx_pathprep_desc* d, const crx_path_desc* qd, int n_scen, const int32_t* active, const double* x_wrapped,
                  const double* x_raw, const int32_t* n_veh, const int32_t* order, const double* veh_xcurv, const double* max_dv,
                  const double* obs_ey, const double* opt_s, const double* opt_ey, const double* opt_vx, double* E, double* cost,
                  int32_t* status, double* kkt, int32_t* iters, int32_t* flag, double* target, int32_t* plan_status) {
    crx_pathplan_kparams chk;
    const arr own = &chk;   // the prep arrays and the QP mask are this call's staging: present by construction
    if (int rc = check_pathplan(chk, d, qd, true, n_scen, x_wrapped, x_raw, n_veh, order, veh_xcurv, max_dv, obs_ey, opt_s, opt_ey, opt_vx, own,
                                own, own, own, own, own, own, own, E, cost, status, kkt, iters, flag, target, plan_status))
        return rc;
    if (n_scen == 0) return CRX_OK;
    if (int rc = check_pathplan_host(d, n_scen, n_veh, order)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    const size_t S = (size_t)n_scen, N1 = (size_t)d->N + 1, V = (size_t)d->n_veh_max, R = V + 1, T = (size_t)d->n_opt;
    const size_t row = (S * R * N1 * sizeof(double) + 255) & ~size_t(255), vec = (S * R * sizeof(double) + 255) & ~size_t(255);
    Stage sg;
    auto dxw = sg.in(x_wrapped, S * 6); auto dxr = sg.in(x_raw, S * 6); auto dnv = sg.in(n_veh, S); auto dor = sg.in(order, S * V);
    auto dvx = sg.in(veh_xcurv, S * (size_t)d->n_all_max * 6); auto dmd = sg.in(max_dv, S); auto doe = sg.in(obs_ey, S * V * N1);
    auto dts = sg.in(opt_s, T); auto dte = sg.in(opt_ey, T); auto dtv = sg.in(opt_vx, T);
    auto dac = active ? sg.in(active, S) : Stage::Ref<int32_t>{};
    // in/out: what a skipped scenario leaves untouched is the caller's data
    auto dE = sg.inout(E, S * R * N1); auto dk = sg.inout(kkt, S * R); auto dtg = sg.inout(target, S * N1 * 6);
    auto dc = sg.out(cost, S * R); auto ds = sg.out(status, S * R); auto di = sg.out(iters, S * R);
    auto dfl = sg.out(flag, S); auto dps = sg.out(plan_status, S);
    auto dws = sg.scratch(4 * row + 4 * vec);   // opt, bez, lb, ub | e0, eN, span (S <= S R), qp_active (4 B each)
    if (int rc = sg.up(g_stream)) return rc;
    char* w = sg[dws];
    double *wopt = (double*)w, *wbez = (double*)(w + row), *wlb = (double*)(w + 2 * row), *wub = (double*)(w + 3 * row);
    double *we0 = (double*)(w + 4 * row), *weN = (double*)(w + 4 * row + vec), *wsp = (double*)(w + 4 * row + 2 * vec);
    int32_t* wqa = (int32_t*)(w + 4 * row + 3 * vec);
    if (int rc = crx_path_plan_dev(d, qd, n_scen, sg[dac], sg[dxw], sg[dxr], sg[dnv], sg[dor], sg[dvx], sg[dmd], sg[doe], sg[dts], sg[dte],
                                   sg[dtv], wopt, wbez, wlb, wub, we0, weN, wsp, wqa, sg[dE], sg[dc], sg[ds], sg[dk], sg[di], sg[dfl], sg[dtg],
                                   sg[dps], g_stream)) return rc;
    return sg.down(g_stream);
}

// ---- plant ----------------------------------------------------------------------------------------
void crx_plant_desc_default(crx_plant_desc* d, int n_seg, double lap_length) {
    memset(d, 0, sizeof(*d));
    d->n_sub = 100; d->n_seg = n_seg; d->dt_sub = 0.001; d->lap_length = lap_length;
    d->m = 1.98; d->lf = 0.125; d->lr = 0.125; d->Iz = 0.024;
    d->Df = 0.8 * 1.98 * 9.81 / 2.0; d->Cf = 1.25; d->Bf = 1.0;
    d->Dr = 0.8 * 1.98 * 9.81 / 2.0; d->Cr = 1.25; d->Br = 1.0;
}

// host_params: the [batch][CRX_PLANT_NPARAM] rows of a host-pointer entry (NULL: none, or on the device where they cannot be read), held to what
// the descriptor's own ten values are held to, and finite
static int check_plant(const crx_plant_desc* d, int batch, int u_stride, arr track, arr xglob, arr xcurv, arr u, arr xglob_next, arr xcurv_next,
                       const double* host_params = nullptr) {
    if (int rc = ensure_init()) return rc;
    if (!d) return fail(CRX_ERR_ARG, "desc is NULL");
    if (d->n_sub < 0 || d->n_seg < 1 || d->n_seg > 64) return fail(CRX_ERR_ARG, "n_sub < 0 or n_seg outside [1,64]");
    if (!(d->lap_length > 0.0) || !(d->m > 0.0) || !(d->Iz > 0.0)) return fail(CRX_ERR_ARG, "lap_length, m, Iz must be positive");
    if (batch < 0) return fail(CRX_ERR_ARG, "batch < 0");
    if (u_stride < 2) return fail(CRX_ERR_ARG, "u_stride < 2");
    if (batch > 0 && any_null(track, xglob, xcurv, u, xglob_next, xcurv_next)) return fail(CRX_ERR_ARG, "NULL array argument");
    for (int b = 0; host_params && b < batch; b++) {
        const double* r = host_params + (size_t)CRX_PLANT_NPARAM * b;
        bool ok = r[0] > 0.0 && r[3] > 0.0;
        for (int i = 0; i < CRX_PLANT_NPARAM; i++) ok = ok && isfinite(r[i]);
        if (!ok) return fail(CRX_ERR_ARG, "params of car %d: m and Iz must be positive, all %d values finite", b, CRX_PLANT_NPARAM);
    }
    return 0;
}

// the one launch behind every plant entry: params NULL = the descriptor's ten values for every vehicle (crx_plant_kernel), else one row per
// vehicle (crx_plant_cars_kernel)
static int plant_launch(const crx_plant_desc* d, int batch, int wrap, const double* track, const double* xglob, const double* xcurv,
                        const double* u, int u_stride, const double* noise_z, const double* params, double* xglob_next, double* xcurv_next,
                        int32_t* laps, void* stream) {
    if (int rc = check_plant(d, batch, u_stride, track, xglob, xcurv, u, xglob_next, xcurv_next)) return rc;
    if (batch == 0) return CRX_OK;
    crx_plant_kparams_cars pk;
    pk.d = *d; pk.batch = batch; pk.u_stride = u_stride; pk.wrap = wrap; pk.track = track; pk.xglob = xglob; pk.xcurv = xcurv; pk.u = u;
    pk.xglob_next = xglob_next; pk.xcurv_next = xcurv_next; pk.laps = laps; pk.noise_z = noise_z; pk.params = params;
    if (params) return launched(crx_launch_plant_cars(pk, (hipStream_t)stream), "plant (per-car parameters)");
    return launched(crx_launch_plant(pk, (hipStream_t)stream), "plant");
}

int crx_plant_step_dev(const crx_plant_desc* d, int batch, const double* track, const double* xglob, const double* xcurv,
                       const double* u, double* xglob_next, double* xcurv_next, void* stream) {
    return plant_launch(d, batch, 0, track, xglob, xcurv, u, 2, nullptr, nullptr, xglob_next, xcurv_next, nullptr, stream);
}

int crx_plant_step_wrap_dev(const crx_plant_desc* d, int batch, const double* track, const double* xglob, const double* xcurv,
                            const double* u, int u_stride, double* xglob_next, double* xcurv_next, int32_t* laps, void* stream) {
    return plant_launch(d, batch, 1, track, xglob, xcurv, u, u_stride, nullptr, nullptr, xglob_next, xcurv_next, laps, stream);
}

int crx_plant_step_noise_dev(const crx_plant_desc* d, int batch, const double* track, const double* xglob, const double* xcurv,
                             const double* u, int u_stride, const double* noise_z, double* xglob_next, double* xcurv_next,
                             int32_t* laps, void* stream) {
    return plant_launch(d, batch, 1, track, xglob, xcurv, u, u_stride, noise_z, nullptr, xglob_next, xcurv_next, laps, stream);
}

int crx_plant_step_params_dev(const crx_plant_desc* d, int batch, const double* track, const double* xglob, const double* xcurv,
                              const double* u, int u_stride, const double* noise_z, const double* params, double* xglob_next,
                              double* xcurv_next, int32_t* laps, void* stream) {
    return plant_launch(d, batch, 1, track, xglob, xcurv, u, u_stride, noise_z, params, xglob_next, xcurv_next, laps, stream);
}

int crx_plant_step_params_plain_dev(const crx_plant_desc* d, int batch, const double* track, const double* xglob, const double* xcurv,
                                    const double* u, const double* params, double* xglob_next, double* xcurv_next, void* stream) {
    return plant_launch(d, batch, 0, track, xglob, xcurv, u, 2, nullptr, params, xglob_next, xcurv_next, nullptr, stream);
}

// ---- one track per car: a track set behind the plant (crx_plant_tracks_kernel), one lap length per race behind the MPC-CBF prep ----
// host_*: the arrays of the host-pointer entry (NULL: on the device, where they cannot be read)
// `batch` ids, one per car (track_id) or, with per_race, one per race (race_track: the field families)
static int check_track_set(int batch, int n_tracks, int seg_stride, arr n_seg, arr lap_length, arr track_id, const int32_t* host_n_seg = nullptr,
                           const double* host_lap = nullptr, const int32_t* host_id = nullptr, bool per_race = false) {
    if (n_tracks < 1 || n_tracks > CRX_MAX_TRACKS) return fail(CRX_ERR_ARG, "n_tracks=%d outside [1,%d]", n_tracks, CRX_MAX_TRACKS);
    if (seg_stride < 1 || seg_stride > CRX_PLANT_MAX_SEG) return fail(CRX_ERR_ARG, "seg_stride=%d outside [1,%d]", seg_stride, CRX_PLANT_MAX_SEG);
    if (batch > 0 && any_null(n_seg, lap_length, track_id)) return fail(CRX_ERR_ARG, "NULL array argument");
    for (int t = 0; host_n_seg && t < n_tracks; t++)
        if (host_n_seg[t] < 1 || host_n_seg[t] > seg_stride) return fail(CRX_ERR_ARG, "n_seg of track %d: %d outside [1,%d]", t, host_n_seg[t], seg_stride);
    for (int t = 0; host_lap && t < n_tracks; t++)
        if (!(host_lap[t] > 0.0) || !isfinite(host_lap[t])) return fail(CRX_ERR_ARG, "lap_length of track %d must be positive and finite", t);
    for (int b = 0; host_id && b < batch; b++)
        if (host_id[b] < 0 || host_id[b] >= n_tracks)
            return fail(CRX_ERR_ARG, "%s %d: %d outside [0,%d)", per_race ? "race_track of race" : "track_id of car", b, host_id[b], n_tracks);
    return 0;
}

static int plant_tracks_launch(const crx_plant_desc* d, int batch, int wrap, int n_tracks, int seg_stride, const double* tracks, const int32_t* n_seg,
                               const double* lap_length, const int32_t* track_id, const double* xglob, const double* xcurv, const double* u,
                               int u_stride, const double* noise_z, const double* params, double* xglob_next, double* xcurv_next, int32_t* laps,
                               void* stream) {
    if (int rc = check_plant(d, batch, u_stride, tracks, xglob, xcurv, u, xglob_next, xcurv_next)) return rc;
    if (int rc = check_track_set(batch, n_tracks, seg_stride, n_seg, lap_length, track_id)) return rc;
    if (batch == 0) return CRX_OK;
    crx_plant_kparams_tracks pk;
    pk.d = *d; pk.batch = batch; pk.u_stride = u_stride; pk.wrap = wrap; pk.track = tracks; pk.xglob = xglob; pk.xcurv = xcurv; pk.u = u;
    pk.xglob_next = xglob_next; pk.xcurv_next = xcurv_next; pk.laps = laps; pk.noise_z = noise_z; pk.params = params;
    pk.n_tracks = n_tracks; pk.seg_stride = seg_stride; pk.n_seg = n_seg; pk.track_id = track_id; pk.lap_length = lap_length;
    return launched(crx_launch_plant_tracks(pk, (hipStream_t)stream), "plant (track set)");
}

int crx_plant_step_tracks_dev(const crx_plant_desc* d, int batch, int n_tracks, int seg_stride, const double* tracks, const int32_t* n_seg,
                              const double* lap_length, const int32_t* track_id, const double* xglob, const double* xcurv, const double* u,
                              int u_stride, const double* noise_z, const double* params, double* xglob_next, double* xcurv_next,
                              int32_t* laps, void* stream) {
    return plant_tracks_launch(d, batch, 1, n_tracks, seg_stride, tracks, n_seg, lap_length, track_id, xglob, xcurv, u, u_stride, noise_z, params,
                               xglob_next, xcurv_next, laps, stream);
}

int crx_plant_step_tracks_plain_dev(const crx_plant_desc* d, int batch, int n_tracks, int seg_stride, const double* tracks,
                                    const int32_t* n_seg, const double* lap_length, const int32_t* track_id, const double* xglob,
                                    const double* xcurv, const double* u, const double* params, double* xglob_next, double* xcurv_next,
                                    void* stream) {
    return plant_tracks_launch(d, batch, 0, n_tracks, seg_stride, tracks, n_seg, lap_length, track_id, xglob, xcurv, u, 2, nullptr, params,
                               xglob_next, xcurv_next, nullptr, stream);
}

int crx_cbf_prep_laps_dev(int N, int V, const double* lap_length, double t, double dt, double safety_time, int batch,
                          const double* xcurv, const double* car_s0, const double* car_v, const double* car_ey,
                          double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs, void* stream) {
    if (int rc = ensure_init()) return rc;
    if (N < 1 || N > CRX_MAX_N || V < 1 || V > CRX_MAX_OBS || batch < 0) return fail(CRX_ERR_ARG, "bad cbf prep dimensions");
    if (batch == 0) return CRX_OK;
    if (!lap_length || !xcurv || !car_s0 || !car_v || !car_ey || !obs_s || !obs_ey || !lap_off || !n_obs) return fail(CRX_ERR_ARG, "NULL array argument");
    crx_cbfprep_kparams_laps cp;
    cp.N = N; cp.V = V; cp.batch = batch; cp.lap_length = 0.0; cp.lap_lengths = lap_length; cp.t = t; cp.dt = dt; cp.safety_time = safety_time;
    cp.xcurv = xcurv; cp.car_s0 = car_s0; cp.car_v = car_v; cp.car_ey = car_ey;
    cp.obs_s = obs_s; cp.obs_ey = obs_ey; cp.lap_off = lap_off; cp.n_obs = n_obs;
    return launched(crx_launch_cbfprep_laps(cp, (hipStream_t)stream), "cbf prep (per-race lap lengths)");
}

int crx_cbf_prep_dev(int N, int V, double lap_length, double t, double dt, double safety_time, int batch,
                     const double* xcurv, const double* car_s0, const double* car_v, const double* car_ey,
                     double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs, void* stream) {
    if (int rc = ensure_init()) return rc;
    if (N < 1 || N > CRX_MAX_N || V < 1 || V > CRX_MAX_OBS || batch < 0 || !(lap_length > 0.0)) return fail(CRX_ERR_ARG, "bad cbf prep dimensions");
    if (batch == 0) return CRX_OK;
    if (!xcurv || !car_s0 || !car_v || !car_ey || !obs_s || !obs_ey || !lap_off || !n_obs) return fail(CRX_ERR_ARG, "NULL array argument");
    crx_cbfprep_kparams cp;
    cp.N = N; cp.V = V; cp.batch = batch; cp.lap_length = lap_length; cp.t = t; cp.dt = dt; cp.safety_time = safety_time;
    cp.xcurv = xcurv; cp.car_s0 = car_s0; cp.car_v = car_v; cp.car_ey = car_ey;
    cp.obs_s = obs_s; cp.obs_ey = obs_ey; cp.lap_off = lap_off; cp.n_obs = n_obs;
    return launched(crx_launch_cbfprep(cp, (hipStream_t)stream), "cbf prep");
}

// ---- field races: every car of a race drives itself (crx_field_prep_kernel, crx_prep.hip) ------------------------------------
void crx_field_desc_default(crx_field_desc* d, int N, int n_cars, int n_seg, double lap_length) {
    memset(d, 0, sizeof(*d));
    d->N = N; d->n_cars = n_cars; d->n_seg = n_seg; d->degree = 6;
    d->lap_length = lap_length; d->dt = 0.1; d->safety_time = 2.0; d->l_sum = 0.4; d->w_sum = 0.2;
}

static bool positive(double v) { return v > 0.0 && isfinite(v); }
// The scalars of crx_field_desc and crx_mixed_desc and the race count, in the order both families refuse them.  A field is a mixed field
// without iLQR cars: its N_ilqr = 0 and ilqr_obstacles = 0 pass the two checks it does not have.
static int check_field_scalars(int N, int N_ilqr, int n_cars, int n_seg, int degree, int ilqr_obstacles, double lap_length, double dt, double l_sum,
                               double w_sum, int n_races) {
    if (N < 1 || N > CRX_MAX_N) return fail(CRX_ERR_ARG, "N=%d outside [1,%d]", N, CRX_MAX_N);
    if (N_ilqr < 0 || N_ilqr > CRX_ILQR_MAX_N) return fail(CRX_ERR_ARG, "N_ilqr=%d outside [0,%d]", N_ilqr, CRX_ILQR_MAX_N);
    if (n_cars < 1 || n_cars > CRX_MAX_OBS + 1) return fail(CRX_ERR_ARG, "n_cars=%d outside [1,%d]", n_cars, CRX_MAX_OBS + 1);
    if (n_seg < 1 || n_seg > CRX_PLANT_MAX_SEG) return fail(CRX_ERR_ARG, "n_seg=%d outside [1,%d]", n_seg, CRX_PLANT_MAX_SEG);
    if (degree < 2 || degree > 8 || (degree & 1)) return fail(CRX_ERR_ARG, "degree must be 2, 4, 6 or 8");
    if (ilqr_obstacles != 0 && ilqr_obstacles != 1) return fail(CRX_ERR_ARG, "ilqr_obstacles=%d must be 0 or 1", ilqr_obstacles);
    if (!positive(lap_length) || !positive(dt) || !positive(l_sum) || !positive(w_sum))
        return fail(CRX_ERR_ARG, "lap_length, dt, l_sum and w_sum must be positive and finite");
    if (n_races < 0) return fail(CRX_ERR_ARG, "n_races < 0");
    return 0;
}

// The arrays of the NLP family (crx_field_prep*, crx_mixed_prep*): arguments alone, so the answer is the same with and without a device.
// null_in: an array every call of the entry needs is NULL; null_ilqr: one of the iLQR family's, refused at its place in crx_mixed_prep*'s
// order.  host_dims: the [n_races][n_cars][2] rows of the host-pointer entry (NULL: none, or on the device where they cannot be read)
static int check_field_arrays(int n_races, int n_cars, int N_ilqr, bool null_in, bool null_ilqr, arr car_dims, arr obs_s, arr obs_ey, arr lap_off,
                              arr obs_dims, const double* host_dims) {
    if (n_cars > 1 && !car_dims != !obs_dims)   // (one car: obs_dims holds nothing, like the other [V] arrays)
        return fail(CRX_ERR_ARG, "car_dims and obs_dims go together: both or neither (%s is NULL)", car_dims ? "obs_dims" : "car_dims");
    if (n_races > 0 && (null_in || (n_cars > 1 && any_null(obs_s, obs_ey, lap_off)))) return fail(CRX_ERR_ARG, "NULL array argument");
    if (n_races > 0 && N_ilqr > 0 && null_ilqr) return fail(CRX_ERR_ARG, "NULL array argument of the iLQR family (N_ilqr=%d)", N_ilqr);
    for (size_t i = 0; host_dims && i < (size_t)n_races * n_cars; i++)
        if (!positive(host_dims[2 * i]) || !positive(host_dims[2 * i + 1]))
            return fail(CRX_ERR_ARG, "car_dims of car %zu of race %zu: length and width must be positive and finite", i % n_cars, i / n_cars);
    return 0;
}

// The descriptor and the race count of both field entry families (crx_field_prep*, crx_field_traffic*)
static int check_field_desc(const crx_field_desc* d, int n_races) {
    if (!d) return fail(CRX_ERR_ARG, "desc is NULL");
    return check_field_scalars(d->N, 0, d->n_cars, d->n_seg, d->degree, 0, d->lap_length, d->dt, d->l_sum, d->w_sum, n_races);
}

static int check_field(crx_field_kparams& fp, const crx_field_desc* d, int n_races, arr track, arr xcurv, arr car_dims, arr pred_s, arr pred_ey,
                       arr obs_s, arr obs_ey, arr lap_off, arr n_obs, arr obs_dims, const double* host_dims = nullptr) {
    if (int rc = check_field_desc(d, n_races)) return rc;
    if (int rc = check_field_arrays(n_races, d->n_cars, 0, any_null(track, xcurv, pred_s, pred_ey, n_obs), false, car_dims, obs_s, obs_ey, lap_off,
                                    obs_dims, host_dims)) return rc;
    memset(&fp, 0, sizeof(fp));
    fp.d = *d; fp.n_races = n_races;
    return 0;
}

int crx_field_prep_dev(const crx_field_desc* d, int n_races, const double* track, const double* xcurv, const double* car_dims, double* pred_s,
                       double* pred_ey, double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs, double* obs_dims, double* clear,
                       void* stream) {
    crx_field_kparams fp;
    if (int rc = check_field(fp, d, n_races, track, xcurv, car_dims, pred_s, pred_ey, obs_s, obs_ey, lap_off, n_obs, obs_dims)) return rc;
    if (int rc = ensure_init()) return rc;
    if (n_races == 0) return CRX_OK;
    fp.track = track; fp.xcurv = xcurv; fp.car_dims = car_dims; fp.pred_s = pred_s; fp.pred_ey = pred_ey;
    fp.nlp = {obs_s, obs_ey, lap_off, n_obs, d->n_cars > 1 ? obs_dims : nullptr, clear};
    return launched(crx_launch_field_prep(fp, (hipStream_t)stream), "field prep");
}

int crx_field_prep(const crx_field_desc* d, int n_races, const double* track, const double* xcurv, const double* car_dims, double* pred_s,
                   double* pred_ey, double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs, double* obs_dims, double* clear) {
    crx_field_kparams chk;
    if (int rc = check_field(chk, d, n_races, track, xcurv, car_dims, pred_s, pred_ey, obs_s, obs_ey, lap_off, n_obs, obs_dims, car_dims)) return rc;
    if (int rc = ensure_init()) return rc;
    if (n_races == 0) return CRX_OK;
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    const size_t RC = (size_t)n_races * d->n_cars, V = (size_t)d->n_cars - 1, N1 = (size_t)d->N + 1;
    Stage sg;
    auto dtr = sg.in(track, (size_t)d->n_seg * 6); auto dx = sg.in(xcurv, RC * 6);
    auto dcd = car_dims ? sg.in(car_dims, RC * 2) : Stage::Ref<double>{};   // unused: sg[dcd] is NULL
    auto dps = sg.out(pred_s, RC * N1); auto dpe = sg.out(pred_ey, RC * N1);
    auto dos = sg.out(obs_s, RC * V * N1); auto doe = sg.out(obs_ey, RC * V * N1); auto dlo = sg.out(lap_off, RC * V);
    auto dno = sg.out(n_obs, RC);
    auto dod = obs_dims ? sg.out(obs_dims, RC * V * 2) : Stage::Ref<double>{};
    auto dcl = clear ? sg.out(clear, RC) : Stage::Ref<double>{};
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_field_prep_dev(d, n_races, sg[dtr], sg[dx], sg[dcd], sg[dps], sg[dpe], sg[dos], sg[doe], sg[dlo], sg[dno], sg[dod], sg[dcl],
                                    g_stream)) return rc;
    return sg.down(g_stream);
}

// ---- field races and mixed fields on one track per RACE (crx_field_prep_tracks_kernel, crx_mixed_prep_tracks_kernel, crx_prep.hip) ----------
// The set's own arrays are read at any race count by the host-pointer entries, as crx_plant_step_tracks reads them
static int check_race_tracks_host(int n_races, int n_tracks, int seg_stride, const int32_t* n_seg, const double* lap_length, const int32_t* race_track) {
    if (n_tracks >= 1 && n_tracks <= CRX_MAX_TRACKS && any_null(n_seg, lap_length)) return fail(CRX_ERR_ARG, "NULL array argument");
    return check_track_set(n_races, n_tracks, seg_stride, n_seg, lap_length, race_track, n_seg, lap_length, n_races > 0 ? race_track : nullptr, true);
}
static crx_race_tracks race_tracks_of(int n_tracks, int seg_stride, const int32_t* n_seg, const double* lap_length, const int32_t* race_track) {
    crx_race_tracks set;
    set.n_tracks = n_tracks; set.seg_stride = seg_stride; set.n_seg = n_seg; set.race_track = race_track; set.lap_length = lap_length;
    return set;
}

int crx_field_prep_tracks_dev(const crx_field_desc* d, int n_races, int n_tracks, int seg_stride, const double* tracks, const int32_t* n_seg,
                              const double* lap_length, const int32_t* race_track, const double* xcurv, const double* car_dims, double* pred_s,
                              double* pred_ey, double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs, double* obs_dims, double* clear,
                              void* stream) {
    crx_field_kparams_tracks fp;
    if (int rc = check_field(fp, d, n_races, tracks, xcurv, car_dims, pred_s, pred_ey, obs_s, obs_ey, lap_off, n_obs, obs_dims)) return rc;
    if (int rc = check_track_set(n_races, n_tracks, seg_stride, n_seg, lap_length, race_track)) return rc;
    if (int rc = ensure_init()) return rc;
    if (n_races == 0) return CRX_OK;
    fp.track = tracks; fp.xcurv = xcurv; fp.car_dims = car_dims; fp.pred_s = pred_s; fp.pred_ey = pred_ey;
    fp.nlp = {obs_s, obs_ey, lap_off, n_obs, d->n_cars > 1 ? obs_dims : nullptr, clear};
    fp.set = race_tracks_of(n_tracks, seg_stride, n_seg, lap_length, race_track);
    return launched(crx_launch_field_prep_tracks(fp, (hipStream_t)stream), "field prep (track set)");
}

int crx_field_prep_tracks(const crx_field_desc* d, int n_races, int n_tracks, int seg_stride, const double* tracks, const int32_t* n_seg,
                          const double* lap_length, const int32_t* race_track, const double* xcurv, const double* car_dims, double* pred_s,
                          double* pred_ey, double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs, double* obs_dims, double* clear) {
    crx_field_kparams_tracks chk;
    if (int rc = check_field(chk, d, n_races, tracks, xcurv, car_dims, pred_s, pred_ey, obs_s, obs_ey, lap_off, n_obs, obs_dims, car_dims)) return rc;
    if (int rc = check_race_tracks_host(n_races, n_tracks, seg_stride, n_seg, lap_length, race_track)) return rc;
    if (int rc = ensure_init()) return rc;
    if (n_races == 0) return CRX_OK;
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    const size_t RC = (size_t)n_races * d->n_cars, V = (size_t)d->n_cars - 1, N1 = (size_t)d->N + 1;
    Stage sg;
    auto dtr = sg.in(tracks, (size_t)n_tracks * seg_stride * 6); auto dns = sg.in(n_seg, (size_t)n_tracks); auto dll = sg.in(lap_length, (size_t)n_tracks);
    auto drt = sg.in(race_track, (size_t)n_races); auto dx = sg.in(xcurv, RC * 6);
    auto dcd = car_dims ? sg.in(car_dims, RC * 2) : Stage::Ref<double>{};   // unused: sg[dcd] is NULL
    auto dps = sg.out(pred_s, RC * N1); auto dpe = sg.out(pred_ey, RC * N1);
    auto dos = sg.out(obs_s, RC * V * N1); auto doe = sg.out(obs_ey, RC * V * N1); auto dlo = sg.out(lap_off, RC * V);
    auto dno = sg.out(n_obs, RC);
    auto dod = obs_dims ? sg.out(obs_dims, RC * V * 2) : Stage::Ref<double>{};
    auto dcl = clear ? sg.out(clear, RC) : Stage::Ref<double>{};
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_field_prep_tracks_dev(d, n_races, n_tracks, seg_stride, sg[dtr], sg[dns], sg[dll], sg[drt], sg[dx], sg[dcd], sg[dps], sg[dpe],
                                           sg[dos], sg[doe], sg[dlo], sg[dno], sg[dod], sg[dcl], g_stream)) return rc;
    return sg.down(g_stream);
}

// ---- field games: the racing game's traffic arrays of a field (crx_field_traffic_kernel, crx_prep.hip) ------------------------------------
static_assert(CRX_MAX_VEH == CRX_MAX_OBS, "check_field_desc bounds n_cars by CRX_MAX_OBS + 1; the scene takes CRX_MAX_VEH vehicles");
static int check_field_traffic(crx_field_traffic_kparams& tp, const crx_field_desc* d, int n_races, arr track, arr xcurv, arr pred_s_car,
                               arr pred_ey_car, arr veh_xcurv, arr pred_s, arr pred_ey, arr n_all) {
    if (int rc = check_field_desc(d, n_races)) return rc;
    if (n_races > 0 && (any_null(track, xcurv, pred_s_car, pred_ey_car, n_all) || (d->n_cars > 1 && any_null(veh_xcurv, pred_s, pred_ey))))
        return fail(CRX_ERR_ARG, "NULL array argument");
    memset(&tp, 0, sizeof(tp));
    tp.d = *d; tp.n_races = n_races;
    return 0;
}

int crx_field_traffic_dev(const crx_field_desc* d, int n_races, const double* track, const double* xcurv, double* pred_s_car,
                          double* pred_ey_car, double* veh_xcurv, double* pred_s, double* pred_ey, int32_t* n_all, void* stream) {
    crx_field_traffic_kparams tp;
    if (int rc = check_field_traffic(tp, d, n_races, track, xcurv, pred_s_car, pred_ey_car, veh_xcurv, pred_s, pred_ey, n_all)) return rc;
    if (int rc = ensure_init()) return rc;
    if (n_races == 0) return CRX_OK;
    tp.track = track; tp.xcurv = xcurv; tp.pred_s_car = pred_s_car; tp.pred_ey_car = pred_ey_car;
    tp.veh_xcurv = veh_xcurv; tp.pred_s = pred_s; tp.pred_ey = pred_ey; tp.n_all = n_all;
    return launched(crx_launch_field_traffic(tp, (hipStream_t)stream), "field traffic");
}

int crx_field_traffic(const crx_field_desc* d, int n_races, const double* track, const double* xcurv, double* pred_s_car, double* pred_ey_car,
                      double* veh_xcurv, double* pred_s, double* pred_ey, int32_t* n_all) {
    crx_field_traffic_kparams chk;
    if (int rc = check_field_traffic(chk, d, n_races, track, xcurv, pred_s_car, pred_ey_car, veh_xcurv, pred_s, pred_ey, n_all)) return rc;
    if (int rc = ensure_init()) return rc;
    if (n_races == 0) return CRX_OK;
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    const size_t RC = (size_t)n_races * d->n_cars, V = (size_t)d->n_cars - 1, N1 = (size_t)d->N + 1;
    Stage sg;
    auto dtr = sg.in(track, (size_t)d->n_seg * 6); auto dx = sg.in(xcurv, RC * 6);
    auto dpsc = sg.out(pred_s_car, RC * N1); auto dpec = sg.out(pred_ey_car, RC * N1);
    auto dvx = sg.out(veh_xcurv, RC * V * 6); auto dps = sg.out(pred_s, RC * V * N1); auto dpe = sg.out(pred_ey, RC * V * N1);
    auto dna = sg.out(n_all, RC);
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_field_traffic_dev(d, n_races, sg[dtr], sg[dx], sg[dpsc], sg[dpec], sg[dvx], sg[dps], sg[dpe], sg[dna], g_stream)) return rc;
    return sg.down(g_stream);
}

// ---- mixed fields: every car of a race under its own controller (crx_mixed_prep_kernel, crx_prep.hip; crx_mixed_commit_kernel, crx_game.hip) ----
void crx_mixed_desc_default(crx_mixed_desc* d, int N, int N_ilqr, int n_cars, int n_seg, double lap_length) {
    memset(d, 0, sizeof(*d));
    d->N = N; d->N_ilqr = N_ilqr; d->n_cars = n_cars; d->n_seg = n_seg; d->degree = 6; d->ilqr_obstacles = 0;
    d->lap_length = lap_length; d->dt = 0.1; d->safety_time = 2.0; d->l_sum = 0.4; d->w_sum = 0.2;
}

// The descriptor and the race count of crx_mixed_prep*
static int check_mixed_desc(const crx_mixed_desc* d, int n_races) {
    if (!d) return fail(CRX_ERR_ARG, "desc is NULL");
    return check_field_scalars(d->N, d->N_ilqr, d->n_cars, d->n_seg, d->degree, d->ilqr_obstacles, d->lap_length, d->dt, d->l_sum, d->w_sum, n_races);
}

// Arguments alone, before the library's state is looked at.  host_dims, host_policy: the rows of the host-pointer entry (NULL: on the device)
static int check_mixed(crx_mixed_kparams& mp, const crx_mixed_desc* d, int n_races, arr track, arr xcurv, arr policy, arr car_dims, arr pred_s,
                       arr pred_ey, arr obs_s, arr obs_ey, arr lap_off, arr n_obs, arr obs_dims, arr m_nlp, arr il_obs_s, arr il_obs_ey,
                       arr il_lap_off, arr il_n_obs, arr m_ilqr, const double* host_dims = nullptr, const int32_t* host_policy = nullptr) {
    if (int rc = check_mixed_desc(d, n_races)) return rc;
    if (int rc = check_field_arrays(n_races, d->n_cars, d->N_ilqr, any_null(track, xcurv, policy, pred_s, pred_ey, n_obs, m_nlp),
                                    any_null(il_n_obs, m_ilqr) || (d->n_cars > 1 && any_null(il_obs_s, il_obs_ey, il_lap_off)), car_dims, obs_s,
                                    obs_ey, lap_off, obs_dims, host_dims)) return rc;
    for (size_t i = 0; host_policy && i < (size_t)n_races * d->n_cars; i++)
        if (host_policy[i] < 0 || host_policy[i] >= CRX_POLICY_COUNT)
            return fail(CRX_ERR_ARG, "policy=%d of car %zu of race %zu outside [0,%d]", host_policy[i], i % d->n_cars, i / d->n_cars, CRX_POLICY_COUNT - 1);
    memset(&mp, 0, sizeof(mp));
    mp.d = *d; mp.n_races = n_races;
    return 0;
}

int crx_mixed_prep_dev(const crx_mixed_desc* d, int n_races, const double* track, const double* xcurv, const int32_t* policy,
                       const double* car_dims, double* pred_s, double* pred_ey, double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs,
                       double* obs_dims, int32_t* m_nlp, double* il_obs_s, double* il_obs_ey, double* il_lap_off, int32_t* il_n_obs,
                       int32_t* m_ilqr, double* clear, void* stream) {
    crx_mixed_kparams mp;
    if (int rc = check_mixed(mp, d, n_races, track, xcurv, policy, car_dims, pred_s, pred_ey, obs_s, obs_ey, lap_off, n_obs, obs_dims, m_nlp,
                             il_obs_s, il_obs_ey, il_lap_off, il_n_obs, m_ilqr)) return rc;
    if (int rc = ensure_init()) return rc;
    if (n_races == 0) return CRX_OK;
    mp.track = track; mp.xcurv = xcurv; mp.policy = policy; mp.car_dims = car_dims; mp.pred_s = pred_s; mp.pred_ey = pred_ey;
    mp.nlp = {obs_s, obs_ey, lap_off, n_obs, d->n_cars > 1 ? obs_dims : nullptr, clear}; mp.m_nlp = m_nlp;
    mp.il_obs_s = il_obs_s; mp.il_obs_ey = il_obs_ey; mp.il_lap_off = il_lap_off; mp.il_n_obs = il_n_obs; mp.m_ilqr = m_ilqr;
    return launched(crx_launch_mixed_prep(mp, (hipStream_t)stream), "mixed prep");
}

int crx_mixed_prep(const crx_mixed_desc* d, int n_races, const double* track, const double* xcurv, const int32_t* policy, const double* car_dims,
                   double* pred_s, double* pred_ey, double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs, double* obs_dims,
                   int32_t* m_nlp, double* il_obs_s, double* il_obs_ey, double* il_lap_off, int32_t* il_n_obs, int32_t* m_ilqr, double* clear) {
    crx_mixed_kparams chk;
    if (int rc = check_mixed(chk, d, n_races, track, xcurv, policy, car_dims, pred_s, pred_ey, obs_s, obs_ey, lap_off, n_obs, obs_dims, m_nlp,
                             il_obs_s, il_obs_ey, il_lap_off, il_n_obs, m_ilqr, car_dims, n_races > 0 ? policy : nullptr)) return rc;
    if (int rc = ensure_init()) return rc;
    if (n_races == 0) return CRX_OK;
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    const size_t RC = (size_t)n_races * d->n_cars, V = (size_t)d->n_cars - 1, N1 = (size_t)d->N + 1, NI1 = (size_t)d->N_ilqr + 1;
    const size_t NP1 = N1 > NI1 ? N1 : NI1, il = d->N_ilqr > 0 ? 1 : 0;   // il = 0: the iLQR family is not staged (the kernel leaves it alone)
    Stage sg;
    auto dtr = sg.in(track, (size_t)d->n_seg * 6); auto dx = sg.in(xcurv, RC * 6); auto dpo = sg.in(policy, RC);
    auto dcd = car_dims ? sg.in(car_dims, RC * 2) : Stage::Ref<double>{};   // unused: sg[dcd] is NULL
    auto dps = sg.out(pred_s, RC * NP1); auto dpe = sg.out(pred_ey, RC * NP1);
    auto dos = sg.out(obs_s, RC * V * N1); auto doe = sg.out(obs_ey, RC * V * N1); auto dlo = sg.out(lap_off, RC * V);
    auto dno = sg.out(n_obs, RC); auto dmn = sg.out(m_nlp, RC);
    auto dod = obs_dims ? sg.out(obs_dims, RC * V * 2) : Stage::Ref<double>{};
    auto dis = il ? sg.out(il_obs_s, RC * V * NI1) : Stage::Ref<double>{}; auto die = il ? sg.out(il_obs_ey, RC * V * NI1) : Stage::Ref<double>{};
    auto dil = il ? sg.out(il_lap_off, RC * V) : Stage::Ref<double>{};
    auto din = il ? sg.out(il_n_obs, RC) : Stage::Ref<int32_t>{}; auto dmi = il ? sg.out(m_ilqr, RC) : Stage::Ref<int32_t>{};
    auto dcl = clear ? sg.out(clear, RC) : Stage::Ref<double>{};
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_mixed_prep_dev(d, n_races, sg[dtr], sg[dx], sg[dpo], sg[dcd], sg[dps], sg[dpe], sg[dos], sg[doe], sg[dlo], sg[dno], sg[dod],
                                    sg[dmn], sg[dis], sg[die], sg[dil], sg[din], sg[dmi], sg[dcl], g_stream)) return rc;
    return sg.down(g_stream);
}

int crx_mixed_prep_tracks_dev(const crx_mixed_desc* d, int n_races, int n_tracks, int seg_stride, const double* tracks, const int32_t* n_seg,
                              const double* lap_length, const int32_t* race_track, const double* xcurv, const int32_t* policy,
                              const double* car_dims, double* pred_s, double* pred_ey, double* obs_s, double* obs_ey, double* lap_off,
                              int32_t* n_obs, double* obs_dims, int32_t* m_nlp, double* il_obs_s, double* il_obs_ey, double* il_lap_off,
                              int32_t* il_n_obs, int32_t* m_ilqr, double* clear, void* stream) {
    crx_mixed_kparams_tracks mp;
    if (int rc = check_mixed(mp, d, n_races, tracks, xcurv, policy, car_dims, pred_s, pred_ey, obs_s, obs_ey, lap_off, n_obs, obs_dims, m_nlp,
                             il_obs_s, il_obs_ey, il_lap_off, il_n_obs, m_ilqr)) return rc;
    if (int rc = check_track_set(n_races, n_tracks, seg_stride, n_seg, lap_length, race_track)) return rc;
    if (int rc = ensure_init()) return rc;
    if (n_races == 0) return CRX_OK;
    mp.track = tracks; mp.xcurv = xcurv; mp.policy = policy; mp.car_dims = car_dims; mp.pred_s = pred_s; mp.pred_ey = pred_ey;
    mp.nlp = {obs_s, obs_ey, lap_off, n_obs, d->n_cars > 1 ? obs_dims : nullptr, clear}; mp.m_nlp = m_nlp;
    mp.il_obs_s = il_obs_s; mp.il_obs_ey = il_obs_ey; mp.il_lap_off = il_lap_off; mp.il_n_obs = il_n_obs; mp.m_ilqr = m_ilqr;
    mp.set = race_tracks_of(n_tracks, seg_stride, n_seg, lap_length, race_track);
    return launched(crx_launch_mixed_prep_tracks(mp, (hipStream_t)stream), "mixed prep (track set)");
}

int crx_mixed_prep_tracks(const crx_mixed_desc* d, int n_races, int n_tracks, int seg_stride, const double* tracks, const int32_t* n_seg,
                          const double* lap_length, const int32_t* race_track, const double* xcurv, const int32_t* policy, const double* car_dims,
                          double* pred_s, double* pred_ey, double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs, double* obs_dims,
                          int32_t* m_nlp, double* il_obs_s, double* il_obs_ey, double* il_lap_off, int32_t* il_n_obs, int32_t* m_ilqr,
                          double* clear) {
    crx_mixed_kparams_tracks chk;
    if (int rc = check_mixed(chk, d, n_races, tracks, xcurv, policy, car_dims, pred_s, pred_ey, obs_s, obs_ey, lap_off, n_obs, obs_dims, m_nlp,
                             il_obs_s, il_obs_ey, il_lap_off, il_n_obs, m_ilqr, car_dims, n_races > 0 ? policy : nullptr)) return rc;
    if (int rc = check_race_tracks_host(n_races, n_tracks, seg_stride, n_seg, lap_length, race_track)) return rc;
    if (int rc = ensure_init()) return rc;
    if (n_races == 0) return CRX_OK;
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    const size_t RC = (size_t)n_races * d->n_cars, V = (size_t)d->n_cars - 1, N1 = (size_t)d->N + 1, NI1 = (size_t)d->N_ilqr + 1;
    const size_t NP1 = N1 > NI1 ? N1 : NI1, il = d->N_ilqr > 0 ? 1 : 0;   // il = 0: the iLQR family is not staged (the kernel leaves it alone)
    Stage sg;
    auto dtr = sg.in(tracks, (size_t)n_tracks * seg_stride * 6); auto dns = sg.in(n_seg, (size_t)n_tracks); auto dll = sg.in(lap_length, (size_t)n_tracks);
    auto drt = sg.in(race_track, (size_t)n_races); auto dx = sg.in(xcurv, RC * 6); auto dpo = sg.in(policy, RC);
    auto dcd = car_dims ? sg.in(car_dims, RC * 2) : Stage::Ref<double>{};   // unused: sg[dcd] is NULL
    auto dps = sg.out(pred_s, RC * NP1); auto dpe = sg.out(pred_ey, RC * NP1);
    auto dos = sg.out(obs_s, RC * V * N1); auto doe = sg.out(obs_ey, RC * V * N1); auto dlo = sg.out(lap_off, RC * V);
    auto dno = sg.out(n_obs, RC); auto dmn = sg.out(m_nlp, RC);
    auto dod = obs_dims ? sg.out(obs_dims, RC * V * 2) : Stage::Ref<double>{};
    auto dis = il ? sg.out(il_obs_s, RC * V * NI1) : Stage::Ref<double>{}; auto die = il ? sg.out(il_obs_ey, RC * V * NI1) : Stage::Ref<double>{};
    auto dil = il ? sg.out(il_lap_off, RC * V) : Stage::Ref<double>{};
    auto din = il ? sg.out(il_n_obs, RC) : Stage::Ref<int32_t>{}; auto dmi = il ? sg.out(m_ilqr, RC) : Stage::Ref<int32_t>{};
    auto dcl = clear ? sg.out(clear, RC) : Stage::Ref<double>{};
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_mixed_prep_tracks_dev(d, n_races, n_tracks, seg_stride, sg[dtr], sg[dns], sg[dll], sg[drt], sg[dx], sg[dpo], sg[dcd], sg[dps],
                                           sg[dpe], sg[dos], sg[doe], sg[dlo], sg[dno], sg[dod], sg[dmn], sg[dis], sg[die], sg[dil], sg[din],
                                           sg[dmi], sg[dcl], g_stream)) return rc;
    return sg.down(g_stream);
}

int crx_mixed_commit_dev(int batch, const int32_t* policy, const double* x, const double* vt, const double* eyt, const double* K,
                         const double* xt, const double* U_nlp, int nlp_stride, const int32_t* nlp_status, const double* U_ilqr,
                         int ilqr_stride, const int32_t* ilqr_status, double* u, int32_t* ctrl_status, void* stream) {
    if (batch < 0) return fail(CRX_ERR_ARG, "batch < 0");
    if (!vt != !eyt || !K != !xt || !U_nlp != !nlp_status || !U_ilqr != !ilqr_status)
        return fail(CRX_ERR_ARG, "the arrays of a family go together: (vt, eyt), (K, xt), (U_nlp, nlp_status), (U_ilqr, ilqr_status), both or neither");
    if ((U_nlp && nlp_stride < 2) || (U_ilqr && ilqr_stride < 2)) return fail(CRX_ERR_ARG, "nlp_stride=%d, ilqr_stride=%d: a given plan has stride >= 2", nlp_stride, ilqr_stride);
    if (batch > 0 && any_null(policy, x, u, ctrl_status)) return fail(CRX_ERR_ARG, "NULL array argument");
    if (int rc = ensure_init()) return rc;
    if (batch == 0) return CRX_OK;
    crx_mixed_commit_kparams cp;
    memset(&cp, 0, sizeof(cp));
    cp.batch = batch; cp.nlp_stride = nlp_stride; cp.ilqr_stride = ilqr_stride; cp.policy = policy; cp.x = x; cp.vt = vt; cp.eyt = eyt; cp.K = K;
    cp.xt = xt; cp.U_nlp = U_nlp; cp.U_ilqr = U_ilqr; cp.nlp_status = nlp_status; cp.ilqr_status = ilqr_status; cp.u = u; cp.ctrl_status = ctrl_status;
    return launched(crx_launch_mixed_commit(cp, (hipStream_t)stream), "mixed commit");
}

int crx_plant_step(const crx_plant_desc* d, int batch, const double* track, const double* xglob, const double* xcurv,
                   const double* u, double* xglob_next, double* xcurv_next) {
    return crx_plant_step_params(d, batch, track, xglob, xcurv, u, nullptr, xglob_next, xcurv_next);
}

int crx_plant_step_params(const crx_plant_desc* d, int batch, const double* track, const double* xglob, const double* xcurv,
                          const double* u, const double* params, double* xglob_next, double* xcurv_next) {
    if (int rc = check_plant(d, batch, 2, track, xglob, xcurv, u, xglob_next, xcurv_next, params)) return rc;
    if (batch == 0) return CRX_OK;
    const size_t B = (size_t)batch;
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    Stage sg;
    auto dtr = sg.in(track, (size_t)d->n_seg * 6); auto dg = sg.in(xglob, B * 6); auto dc = sg.in(xcurv, B * 6); auto du = sg.in(u, B * 2);
    auto dpr = params ? sg.in(params, B * CRX_PLANT_NPARAM) : Stage::Ref<double>{};   // unused: sg[dpr] is NULL
    auto dgn = sg.out(xglob_next, B * 6); auto dcn = sg.out(xcurv_next, B * 6);
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_plant_step_params_plain_dev(d, batch, sg[dtr], sg[dg], sg[dc], sg[du], sg[dpr], sg[dgn], sg[dcn], g_stream)) return rc;
    return sg.down(g_stream);
}

int crx_plant_step_tracks(const crx_plant_desc* d, int batch, int n_tracks, int seg_stride, const double* tracks, const int32_t* n_seg,
                          const double* lap_length, const int32_t* track_id, const double* xglob, const double* xcurv, const double* u,
                          const double* params, double* xglob_next, double* xcurv_next) {
    if (n_tracks >= 1 && n_tracks <= CRX_MAX_TRACKS && !n_seg) return fail(CRX_ERR_ARG, "NULL array argument");   // the set's own arrays are read at any batch
    if (n_tracks >= 1 && n_tracks <= CRX_MAX_TRACKS && !lap_length) return fail(CRX_ERR_ARG, "NULL array argument");
    if (int rc = check_track_set(batch, n_tracks, seg_stride, n_seg, lap_length, track_id, n_seg, lap_length, batch > 0 ? track_id : nullptr)) return rc;
    if (int rc = check_plant(d, batch, 2, tracks, xglob, xcurv, u, xglob_next, xcurv_next, params)) return rc;
    if (batch == 0) return CRX_OK;
    const size_t B = (size_t)batch;
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    Stage sg;
    auto dtr = sg.in(tracks, (size_t)n_tracks * seg_stride * 6); auto dns = sg.in(n_seg, (size_t)n_tracks); auto dll = sg.in(lap_length, (size_t)n_tracks);
    auto dti = sg.in(track_id, B); auto dg = sg.in(xglob, B * 6); auto dc = sg.in(xcurv, B * 6); auto du = sg.in(u, B * 2);
    auto dpr = params ? sg.in(params, B * CRX_PLANT_NPARAM) : Stage::Ref<double>{};   // unused: sg[dpr] is NULL
    auto dgn = sg.out(xglob_next, B * 6); auto dcn = sg.out(xcurv_next, B * 6);
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_plant_step_tracks_plain_dev(d, batch, n_tracks, seg_stride, sg[dtr], sg[dns], sg[dll], sg[dti], sg[dg], sg[dc], sg[du], sg[dpr],
                                                 sg[dgn], sg[dcn], g_stream)) return rc;
    return sg.down(g_stream);
}

// ---- planner host prep on the device ---------------------------------------------------------------
void crx_prep_desc_default(crx_prep_desc* d, int N, int n_veh_max, int n_opt, double track_width, double lap_length) {
    memset(d, 0, sizeof(*d));
    d->N = N; d->n_veh_max = n_veh_max; d->n_opt = n_opt;
    d->prediction_factor = 0.5; d->lookahead = 4.0; d->track_width = track_width; d->lap_length = lap_length;
    d->veh_length = 0.4; d->veh_width = 0.2; d->safety_margin = 0.15; d->dt_ref = 0.1;
}

static int fill_prep(crx_prep_kparams& pp, const crx_prep_desc* d, int n_scen) {
    if (!d) return fail(CRX_ERR_ARG, "desc is NULL");
    if (d->N < 3 || d->N > CRX_MAX_N) return fail(CRX_ERR_ARG, "N=%d outside [3,%d]", d->N, CRX_MAX_N);
    if (d->n_veh_max < 0 || d->n_veh_max > CRX_MAX_VEH) return fail(CRX_ERR_ARG, "n_veh_max=%d outside [0,%d]", d->n_veh_max, CRX_MAX_VEH);
    if (d->n_opt < 2) return fail(CRX_ERR_ARG, "n_opt < 2");
    if (n_scen < 0) return fail(CRX_ERR_ARG, "n_scen < 0");
    if (!(d->lap_length > 0.0) || !(d->track_width > 0.0)) return fail(CRX_ERR_ARG, "lap_length and track_width must be positive");
    memset(&pp, 0, sizeof(pp));
    pp.N = d->N; pp.V = d->n_veh_max; pp.n_scen = n_scen; pp.n_opt = d->n_opt;
    pp.prediction_factor = d->prediction_factor; pp.lookahead = d->lookahead; pp.track_width = d->track_width;
    pp.lap_length = d->lap_length; pp.veh_length = d->veh_length; pp.veh_width = d->veh_width;
    pp.safety_margin = d->safety_margin; pp.dt_ref = d->dt_ref;
    return 0;
}

static int check_prep(crx_prep_kparams& pp, const crx_prep_desc* d, int n_scen, arr x_wrapped, arr x_raw, arr n_veh, arr veh_info, arr max_dv,
                      arr obs_s, arr obs_ey, arr opt_s, arr opt_ey, arr x0, arr bez_s, arr bez_ey, arr ey_lb, arr ey_ub) {
    if (int rc = ensure_init()) return rc;
    if (int rc = fill_prep(pp, d, n_scen)) return rc;
    if (n_scen > 0 && (any_null(x_wrapped, x_raw, n_veh, max_dv, opt_s, opt_ey, x0, bez_s, bez_ey, ey_lb, ey_ub) ||
                       (d->n_veh_max > 0 && any_null(veh_info, obs_s, obs_ey))))
        return fail(CRX_ERR_ARG, "NULL array argument");
    return 0;
}

int crx_planner_prep_dev(const crx_prep_desc* d, int n_scen, const double* x_wrapped, const double* x_raw,
                         const int32_t* n_veh, const double* veh_info, const double* max_dv, const double* obs_s,
                         const double* obs_ey, const double* opt_s, const double* opt_ey, double* x0, double* bez_s,
                         double* bez_ey, double* ey_lb, double* ey_ub, void* stream) {
    crx_prep_kparams pp;
    if (int rc = check_prep(pp, d, n_scen, x_wrapped, x_raw, n_veh, veh_info, max_dv, obs_s, obs_ey, opt_s, opt_ey, x0, bez_s, bez_ey, ey_lb,
                            ey_ub)) return rc;
    if (n_scen == 0) return CRX_OK;
    pp.x_wrapped = x_wrapped; pp.x_raw = x_raw; pp.n_veh = n_veh; pp.veh_info = veh_info; pp.max_dv = max_dv;
    pp.obs_s = obs_s; pp.obs_ey = obs_ey; pp.opt_s = opt_s; pp.opt_ey = opt_ey;
    pp.x0 = x0; pp.bez_s = bez_s; pp.bez_ey = bez_ey; pp.ey_lb = ey_lb; pp.ey_ub = ey_ub;
    return launched(crx_launch_prep(pp, (hipStream_t)stream), "prep");
}

int crx_planner_prep(const crx_prep_desc* d, int n_scen, const double* x_wrapped, const double* x_raw,
                     const int32_t* n_veh, const double* veh_info, const double* max_dv, const double* obs_s,
                     const double* obs_ey, const double* opt_s, const double* opt_ey, double* x0, double* bez_s,
                     double* bez_ey, double* ey_lb, double* ey_ub) {
    crx_prep_kparams chk;
    if (int rc = check_prep(chk, d, n_scen, x_wrapped, x_raw, n_veh, veh_info, max_dv, obs_s, obs_ey, opt_s, opt_ey, x0, bez_s, bez_ey, ey_lb,
                            ey_ub)) return rc;
    if (n_scen == 0) return CRX_OK;
    for (int i = 0; i < n_scen; i++)
        if (n_veh[i] < 0 || n_veh[i] > d->n_veh_max) return fail(CRX_ERR_ARG, "n_veh[%d]=%d outside [0,%d]", i, n_veh[i], d->n_veh_max);
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    const size_t S = (size_t)n_scen, N = (size_t)d->N, V = (size_t)d->n_veh_max, R = V + 1, T = (size_t)d->n_opt;
    const size_t n_ob = S * V * (N + 1), n_bz = S * R * (N + 1);
    Stage sg;
    auto dxw = sg.in(x_wrapped, S * 6); auto dxr = sg.in(x_raw, S * 6); auto dmd = sg.in(max_dv, S);
    auto dvi = sg.in(veh_info, S * V * 3); auto dos = sg.in(obs_s, n_ob); auto doe = sg.in(obs_ey, n_ob);
    auto dts = sg.in(opt_s, T); auto dte = sg.in(opt_ey, T); auto dnv = sg.in(n_veh, S);
    auto dx0 = sg.out(x0, S * R * 6); auto dbs = sg.out(bez_s, n_bz); auto dbe = sg.out(bez_ey, n_bz);
    auto dlb = sg.out(ey_lb, S * R * N); auto dub = sg.out(ey_ub, S * R);
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_planner_prep_dev(d, n_scen, sg[dxw], sg[dxr], sg[dnv], sg[dvi], sg[dmd], sg[dos], sg[doe], sg[dts], sg[dte], sg[dx0],
                                      sg[dbs], sg[dbe], sg[dlb], sg[dub], g_stream)) return rc;
    return sg.down(g_stream);
}

// ---- learning-MPC QP ------------------------------------------------------------------------------
void crx_lmpc_desc_default(crx_lmpc_desc* d, int N, int n_ss_max) {
    memset(d, 0, sizeof(*d));
    d->N = N; d->n_ss_max = n_ss_max;
    d->R[0] = 1.0; d->R[1] = 0.25; d->dR[0] = 4.0; d->dR[1] = 0.0; d->x_track[0] = 5.0;
    d->v_max = 10.0; d->ey_max = 1.0; d->delta_max = 0.5; d->a_max = 1.0; d->w_x0 = 1e4;
    crx_ipm_opts_default(&d->opts);
}

static int fill_lmpc(crx_lmpc_kparams& kp, const crx_lmpc_desc* d, int batch) {
    if (!d) return fail(CRX_ERR_ARG, "desc is NULL");
    if (d->N < 2 || d->N > CRX_LMPC_MAX_N) return fail(CRX_ERR_ARG, "N=%d outside [2,%d]", d->N, CRX_LMPC_MAX_N);
    if (d->n_ss_max < 1 || d->n_ss_max > CRX_MAX_SS) return fail(CRX_ERR_ARG, "n_ss_max=%d outside [1,%d]", d->n_ss_max, CRX_MAX_SS);
    if (batch < 0) return fail(CRX_ERR_ARG, "batch < 0");
    if (!(d->R[0] > 0.0 && d->R[1] > 0.0) || d->dR[0] < 0.0 || d->dR[1] < 0.0) return fail(CRX_ERR_ARG, "R must be positive, dR non-negative");
    for (int c = 0; c < 6; c++)
        if (d->Q[c] < 0.0) return fail(CRX_ERR_ARG, "Q must be non-negative");
    if (!(d->w_x0 > 0.0)) return fail(CRX_ERR_ARG, "w_x0 must be positive");
    if (int rc = check_opts(d->opts)) return rc;
    memset(&kp, 0, sizeof(kp));
    kp.N = d->N; kp.batch = batch; kp.n_ss_max = d->n_ss_max;
    memcpy(kp.Q, d->Q, sizeof(kp.Q)); memcpy(kp.R, d->R, sizeof(kp.R)); memcpy(kp.dR, d->dR, sizeof(kp.dR));
    memcpy(kp.x_track, d->x_track, sizeof(kp.x_track));
    kp.v_max = d->v_max; kp.ey_max = d->ey_max; kp.delta_max = d->delta_max; kp.a_max = d->a_max;
    kp.w_x0 = d->w_x0; kp.opts = d->opts;
    return 0;
}

static int check_lmpc(crx_lmpc_kparams& kp, const crx_lmpc_desc* d, int batch, arr x0, arr u_old, arr A, arr B, arr C, arr ss, arr qfun, arr n_ss,
                      arr X, arr U, arr lambda, arr cost, arr status, arr kkt, arr iters) {
    if (int rc = ensure_init()) return rc;
    if (int rc = fill_lmpc(kp, d, batch)) return rc;
    if (batch > 0 && any_null(x0, u_old, A, B, C, ss, qfun, n_ss, X, U, lambda, cost, status, kkt, iters))
        return fail(CRX_ERR_ARG, "NULL array argument");
    return 0;
}

// n_ss[] is validated on the device side of the boundary only by clamping is NOT acceptable (it indexes
// LDS), so the host entry point checks it; the _dev variant documents the precondition 1 <= n_ss <= n_ss_max.
int crx_lmpc_solve_dev(const crx_lmpc_desc* d, int batch, const double* x0, const double* u_old, const double* A,
                       const double* B, const double* C, const double* ss, const double* qfun, const int32_t* n_ss,
                       double* X, double* U, double* lambda, double* cost, int32_t* status, double* kkt,
                       int32_t* iters, void* stream) {
    return crx_lmpc_solve_masked_dev(d, batch, nullptr, x0, u_old, A, B, C, ss, qfun, n_ss, X, U, lambda, cost, status, kkt, iters, stream);
}

int crx_lmpc_solve_masked_dev(const crx_lmpc_desc* d, int batch, const int32_t* active, const double* x0, const double* u_old,
                              const double* A, const double* B, const double* C, const double* ss, const double* qfun,
                              const int32_t* n_ss, double* X, double* U, double* lambda, double* cost, int32_t* status,
                              double* kkt, int32_t* iters, void* stream) {
    return crx_lmpc_solve_ordered_dev(d, batch, active, nullptr, x0, u_old, A, B, C, ss, qfun, n_ss, X, U, lambda, cost, status, kkt, iters, stream);
}

int crx_lmpc_solve_ordered_dev(const crx_lmpc_desc* d, int batch, const int32_t* active, const int32_t* order, const double* x0,
                               const double* u_old, const double* A, const double* B, const double* C, const double* ss,
                               const double* qfun, const int32_t* n_ss, double* X, double* U, double* lambda, double* cost,
                               int32_t* status, double* kkt, int32_t* iters, void* stream) {
    crx_lmpc_kparams kp;
    if (int rc = check_lmpc(kp, d, batch, x0, u_old, A, B, C, ss, qfun, n_ss, X, U, lambda, cost, status, kkt, iters)) return rc;
    if (batch == 0) return CRX_OK;
    kp.x0 = x0; kp.u_old = u_old; kp.A = A; kp.B = B; kp.C = C; kp.ss = ss; kp.qfun = qfun; kp.n_ss = n_ss;
    kp.X = X; kp.U = U; kp.lambda = lambda; kp.cost = cost; kp.status = status; kp.kkt = kkt; kp.iters = iters;
    kp.active = active; kp.order = order; kp.reach_screen = d->opts.reach_screen ? 1 : 0;
    apply_diagnostics(kp);
    return launched(crx_launch_lmpc(kp, (hipStream_t)stream), "lmpc");
}

int crx_lmpc_solve(const crx_lmpc_desc* d, int batch, const double* x0, const double* u_old, const double* A,
                   const double* B, const double* C, const double* ss, const double* qfun, const int32_t* n_ss,
                   double* X, double* U, double* lambda, double* cost, int32_t* status, double* kkt, int32_t* iters) {
    crx_lmpc_kparams chk;
    if (int rc = check_lmpc(chk, d, batch, x0, u_old, A, B, C, ss, qfun, n_ss, X, U, lambda, cost, status, kkt, iters)) return rc;
    if (batch == 0) return CRX_OK;
    for (int b = 0; b < batch; b++)
        if (n_ss[b] < 1 || n_ss[b] > d->n_ss_max) return fail(CRX_ERR_ARG, "n_ss[%d]=%d outside [1,%d]", b, n_ss[b], d->n_ss_max);
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    const size_t Bn = (size_t)batch, N = (size_t)d->N, M = (size_t)d->n_ss_max;
    Stage sg;
    auto dx0 = sg.in(x0, Bn * 6); auto duo = sg.in(u_old, Bn * 2);
    auto dA = sg.in(A, Bn * N * 36); auto dB = sg.in(B, Bn * N * 12); auto dC = sg.in(C, Bn * N * 6);
    auto dss = sg.in(ss, Bn * 6 * M); auto dq = sg.in(qfun, Bn * M); auto dn = sg.in(n_ss, Bn);
    auto dX = sg.out(X, Bn * (N + 1) * 6); auto dU = sg.out(U, Bn * N * 2); auto dl = sg.out(lambda, Bn * M);
    auto dc = sg.out(cost, Bn); auto dk = sg.out(kkt, Bn); auto ds = sg.out(status, Bn); auto di = sg.out(iters, Bn);
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_lmpc_solve_dev(d, batch, sg[dx0], sg[duo], sg[dA], sg[dB], sg[dC], sg[dss], sg[dq], sg[dn], sg[dX], sg[dU], sg[dl],
                                    sg[dc], sg[ds], sg[dk], sg[di], g_stream)) return rc;
    return sg.down(g_stream);
}

// ---- iLQR (control/control.py:64-195) -----------------------------------------------------------------
void crx_ilqr_desc_default(crx_ilqr_desc* d, int N, const double* A, const double* B) {
    memset(d, 0, sizeof(*d));
    d->N = N; d->max_iter = 150; d->n_obs_max = 1;
    if (A) memcpy(d->A, A, sizeof(d->A));
    if (B) memcpy(d->B, B, sizeof(d->B));
    d->Q[0] = 10.0; d->Q[3 * 7] = 4.0; d->Q[5 * 7] = 40.0;
    d->R[0] = 0.1; d->R[3] = 0.1;
    d->eps = 0.01; d->lamb_init = 1.0; d->lamb_factor = 10.0; d->lamb_max = 1000.0;
    d->margin = 0.15; d->q1 = 2.5; d->q2 = 2.5; d->l_sum = 0.4; d->w_sum = 0.2;
}

// argument checks come before the device check: a malformed call is reported as such with or without a GPU
static int fill_ilqr(crx_ilqr_kparams& kp, const crx_ilqr_desc* d, int batch) {
    if (!d) return fail(CRX_ERR_ARG, "desc is NULL");
    if (d->N < 1 || d->N > CRX_ILQR_MAX_N) return fail(CRX_ERR_ARG, "N=%d outside [1,%d]", d->N, CRX_ILQR_MAX_N);
    if (d->n_obs_max < 0 || d->n_obs_max > CRX_MAX_OBS) return fail(CRX_ERR_ARG, "n_obs_max=%d outside [0,%d]", d->n_obs_max, CRX_MAX_OBS);
    if (d->max_iter < 0) return fail(CRX_ERR_ARG, "max_iter < 0");
    if (batch < 0) return fail(CRX_ERR_ARG, "batch < 0");
    if (!(d->lamb_init > 0.0) || !(d->lamb_factor > 0.0) || !(d->eps >= 0.0)) return fail(CRX_ERR_ARG, "lamb_init, lamb_factor must be positive, eps non-negative");
    if (d->n_obs_max > 0 && !(d->l_sum > 0.0 && d->w_sum > 0.0)) return fail(CRX_ERR_ARG, "l_sum, w_sum must be positive");
    memset(&kp, 0, sizeof(kp));
    kp.N = d->N; kp.batch = batch; kp.n_obs_max = d->n_obs_max; kp.max_iter = d->max_iter;
    memcpy(kp.A, d->A, sizeof(kp.A)); memcpy(kp.B, d->B, sizeof(kp.B)); memcpy(kp.Q, d->Q, sizeof(kp.Q)); memcpy(kp.R, d->R, sizeof(kp.R));
    kp.eps = d->eps; kp.lamb_init = d->lamb_init; kp.lamb_factor = d->lamb_factor; kp.lamb_max = d->lamb_max;
    kp.margin = d->margin; kp.q1 = d->q1; kp.q2 = d->q2; kp.l_sum = d->l_sum; kp.w_sum = d->w_sum;
    return 0;
}

static int check_ilqr(crx_ilqr_kparams& kp, const crx_ilqr_desc* d, int batch, arr x0, arr xt, arr obs_s, arr obs_ey, arr lap_off, arr n_obs, arr X,
                      arr U, arr cost, arr status, arr iters) {
    if (int rc = fill_ilqr(kp, d, batch)) return rc;
    if (batch > 0 && (any_null(x0, xt, n_obs, X, U, cost, status, iters) || (d->n_obs_max > 0 && any_null(obs_s, obs_ey, lap_off))))
        return fail(CRX_ERR_ARG, "NULL array argument");
    return 0;
}

// model_A, model_B [batch][36], [batch][12]: per-problem models, both or neither (neither: d->A, d->B for the whole batch)
static int check_ilqr_models(int batch, arr model_A, arr model_B) {
    if (batch > 0 && !model_A != !model_B) return fail(CRX_ERR_ARG, "NULL array argument (model_A and model_B go together)");
    return 0;
}

int crx_ilqr_solve_models_dev(const crx_ilqr_desc* d, int batch, const int32_t* active, const double* x0, const double* model_A,
                              const double* model_B, const double* xt, const double* obs_s, const double* obs_ey,
                              const double* lap_off, const int32_t* n_obs, double* X, double* U, double* cost, int32_t* status,
                              int32_t* iters, void* stream) {
    crx_ilqr_kparams kp;
    if (int rc = check_ilqr(kp, d, batch, x0, xt, obs_s, obs_ey, lap_off, n_obs, X, U, cost, status, iters)) return rc;
    if (int rc = check_ilqr_models(batch, model_A, model_B)) return rc;
    if (int rc = ensure_init()) return rc;
    if (batch == 0) return CRX_OK;
    kp.x0 = x0; kp.xt = xt; kp.obs_s = obs_s; kp.obs_ey = obs_ey; kp.lap_off = lap_off; kp.n_obs = n_obs; kp.active = active;
    kp.X = X; kp.U = U; kp.cost = cost; kp.status = status; kp.iters = iters;
    kp.model_A = model_A; kp.model_B = model_B;
    return launched(crx_launch_ilqr(kp, (hipStream_t)stream), "ilqr");
}

int crx_ilqr_solve_dev(const crx_ilqr_desc* d, int batch, const int32_t* active, const double* x0, const double* xt,
                       const double* obs_s, const double* obs_ey, const double* lap_off, const int32_t* n_obs, double* X, double* U,
                       double* cost, int32_t* status, int32_t* iters, void* stream) {
    return crx_ilqr_solve_models_dev(d, batch, active, x0, nullptr, nullptr, xt, obs_s, obs_ey, lap_off, n_obs, X, U, cost, status, iters,
                                     stream);
}

int crx_ilqr_solve_models(const crx_ilqr_desc* d, int batch, const double* x0, const double* model_A, const double* model_B,
                          const double* xt, const double* obs_s, const double* obs_ey, const double* lap_off, const int32_t* n_obs,
                          double* X, double* U, double* cost, int32_t* status, int32_t* iters) {
    crx_ilqr_kparams chk;
    if (int rc = check_ilqr(chk, d, batch, x0, xt, obs_s, obs_ey, lap_off, n_obs, X, U, cost, status, iters)) return rc;
    if (int rc = check_ilqr_models(batch, model_A, model_B)) return rc;
    for (int b = 0; b < batch; b++)
        if (n_obs[b] < 0 || n_obs[b] > d->n_obs_max) return fail(CRX_ERR_ARG, "n_obs[%d]=%d outside [0,%d]", b, n_obs[b], d->n_obs_max);
    if (int rc = ensure_init()) return rc;
    if (batch == 0) return CRX_OK;
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    const size_t Bn = (size_t)batch, N = (size_t)d->N, V = (size_t)d->n_obs_max;
    Stage sg;
    auto dx0 = sg.in(x0, Bn * 6); auto dxt = sg.in(xt, Bn * 6);
    auto dos = sg.in(obs_s, Bn * V * (N + 1)); auto doe = sg.in(obs_ey, Bn * V * (N + 1)); auto dlo = sg.in(lap_off, Bn * V);
    auto dn = sg.in(n_obs, Bn);
    auto dmA = model_A ? sg.in(model_A, Bn * 36) : Stage::Ref<double>{};
    auto dmB = model_B ? sg.in(model_B, Bn * 12) : Stage::Ref<double>{};
    auto dX = sg.out(X, Bn * (N + 1) * 6); auto dU = sg.out(U, Bn * N * 2); auto dc = sg.out(cost, Bn);
    auto ds = sg.out(status, Bn); auto di = sg.out(iters, Bn);
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_ilqr_solve_models_dev(d, batch, nullptr, sg[dx0], sg[dmA], sg[dmB], sg[dxt], sg[dos], sg[doe], sg[dlo], sg[dn], sg[dX],
                                           sg[dU], sg[dc], sg[ds], sg[di], g_stream)) return rc;
    return sg.down(g_stream);
}

int crx_ilqr_solve(const crx_ilqr_desc* d, int batch, const double* x0, const double* xt, const double* obs_s, const double* obs_ey,
                   const double* lap_off, const int32_t* n_obs, double* X, double* U, double* cost, int32_t* status, int32_t* iters) {
    return crx_ilqr_solve_models(d, batch, x0, nullptr, nullptr, xt, obs_s, obs_ey, lap_off, n_obs, X, U, cost, status, iters);
}

// ---- LQR design and control law (control/control.py:28-61) ---------------------------------------------------------------
void crx_lqr_desc_default(crx_lqr_desc* d) {
    memset(d, 0, sizeof(*d));
    d->max_iter = 50;
    d->Q[0] = 10.0; d->Q[3 * 7] = 4.0; d->Q[5 * 7] = 40.0;
    d->R[0] = 0.1; d->R[3] = 0.1;
    d->eps = 0.01;
}

static int check_lqr(crx_lqr_kparams& kp, const crx_lqr_desc* d, int batch, arr A, arr B, arr K, arr iters, arr status) {
    if (!d) return fail(CRX_ERR_ARG, "desc is NULL");
    if (d->max_iter < 0) return fail(CRX_ERR_ARG, "max_iter < 0");
    if (batch < 0) return fail(CRX_ERR_ARG, "batch < 0");
    if (batch > 0 && any_null(A, B, K, iters, status)) return fail(CRX_ERR_ARG, "NULL array argument");
    memset(&kp, 0, sizeof(kp));
    kp.batch = batch; kp.max_iter = d->max_iter; kp.eps = d->eps;
    memcpy(kp.Q, d->Q, sizeof(kp.Q)); memcpy(kp.R, d->R, sizeof(kp.R));
    return 0;
}

int crx_lqr_design_dev(const crx_lqr_desc* d, int batch, const int32_t* active, const double* A, const double* B, double* K, double* P,
                       int32_t* iters, int32_t* status, void* stream) {
    crx_lqr_kparams kp;
    if (int rc = check_lqr(kp, d, batch, A, B, K, iters, status)) return rc;
    if (int rc = ensure_init()) return rc;
    if (batch == 0) return CRX_OK;
    kp.A = A; kp.B = B; kp.active = active; kp.K = K; kp.P = P; kp.iters = iters; kp.status = status;
    return launched(crx_launch_lqr_design(kp, (hipStream_t)stream), "lqr design");
}

int crx_lqr_design(const crx_lqr_desc* d, int batch, const double* A, const double* B, double* K, double* P, int32_t* iters,
                   int32_t* status) {
    crx_lqr_kparams chk;
    if (int rc = check_lqr(chk, d, batch, A, B, K, iters, status)) return rc;
    if (int rc = ensure_init()) return rc;
    if (batch == 0) return CRX_OK;
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    const size_t Bn = (size_t)batch;
    Stage sg;
    auto dA = sg.in(A, Bn * 36); auto dB = sg.in(B, Bn * 12);
    auto dK = sg.out(K, Bn * 12); auto dP = P ? sg.out(P, Bn * 36) : Stage::Ref<double>{};
    auto di = sg.out(iters, Bn); auto ds = sg.out(status, Bn);
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_lqr_design_dev(d, batch, nullptr, sg[dA], sg[dB], sg[dK], sg[dP], sg[di], sg[ds], g_stream)) return rc;
    return sg.down(g_stream);
}

int crx_lqr_step_dev(int batch, const double* K, const double* xcurv, const double* xt, double* u, void* stream) {
    if (batch < 0) return fail(CRX_ERR_ARG, "batch < 0");
    if (batch > 0 && any_null(K, xcurv, xt, u)) return fail(CRX_ERR_ARG, "NULL array argument");
    if (int rc = ensure_init()) return rc;
    if (batch == 0) return CRX_OK;
    return launched(crx_launch_lqr_step(batch, K, xcurv, xt, u, (hipStream_t)stream), "lqr step");
}

// ---- LTI system identification (system/system_identification.py:4-43) --------------------------------------------------
void crx_sysid_desc_default(crx_sysid_desc* d) {
    memset(d, 0, sizeof(*d));
    d->lamb = 1e-9; d->first_row = 1; d->chunk_rows = 8192;
}

static int sysid_tpl(const crx_sysid_desc* d, int64_t max_log_rows) {
    const int64_t pairs = max_log_rows - 1 - d->first_row;
    const int64_t t = pairs > 0 ? (pairs + d->chunk_rows - 1) / d->chunk_rows : 0;
    return t > 1 ? (int)t : 1;
}

// max_log_rows: the _dev caller's; the host-pointer entry point derives its own from log_offset AFTER this check and passes 0 here
static int check_sysid(const crx_sysid_desc* d, int n_logs, arr log_offset, arr group_offset, int n_groups, int64_t max_log_rows, arr A, arr B,
                       arr err, arr n_pairs, arr status) {
    if (!d) return fail(CRX_ERR_ARG, "desc is NULL");
    if (!(d->lamb >= 0.0) || !isfinite(d->lamb)) return fail(CRX_ERR_ARG, "lamb must be finite and non-negative");
    if (d->first_row < 0) return fail(CRX_ERR_ARG, "first_row < 0");
    if (d->chunk_rows < 256 || d->chunk_rows > 65536 || d->chunk_rows % 256) return fail(CRX_ERR_ARG, "chunk_rows=%d: a multiple of 256 in [256, 65536]", d->chunk_rows);
    if (n_logs < 0 || n_groups < 0) return fail(CRX_ERR_ARG, "n_logs, n_groups must be >= 0");
    if (!group_offset && n_groups != n_logs) return fail(CRX_ERR_ARG, "group_offset NULL needs n_groups == n_logs");
    if (max_log_rows < 0) return fail(CRX_ERR_ARG, "max_log_rows < 0");
    if ((int64_t)n_logs * sysid_tpl(d, max_log_rows) > INT32_MAX) return fail(CRX_ERR_ARG, "n_logs * tiles per log exceeds the grid");
    if (n_groups > 0 && any_null(log_offset, A, B, err, n_pairs, status)) return fail(CRX_ERR_ARG, "NULL array argument");
    return 0;
}

size_t crx_sysid_workspace_bytes(const crx_sysid_desc* d, int n_logs, int n_groups, int64_t max_log_rows) {
    if (!d || d->chunk_rows <= 0 || n_logs < 0 || n_groups < 0) return 0;
    const size_t tiles = (size_t)n_logs * (size_t)sysid_tpl(d, max_log_rows);
    return (tiles * (84 + 12) + (size_t)n_groups * 48) * sizeof(double) + 2 * 256;
}

int crx_sysid_fit_dev(const crx_sysid_desc* d, int n_logs, const int64_t* log_offset, const int32_t* group_offset, int n_groups,
                      int64_t max_log_rows, const double* x, const double* u, void* workspace, size_t ws_bytes, double* A, double* B,
                      double* err, int64_t* n_pairs, int32_t* status, void* stream) {
    if (int rc = check_sysid(d, n_logs, log_offset, group_offset, n_groups, max_log_rows, A, B, err, n_pairs, status)) return rc;
    const int tpl = sysid_tpl(d, max_log_rows);
    if (n_groups > 0 && !workspace) return fail(CRX_ERR_ARG, "NULL array argument");
    if (n_groups > 0 && max_log_rows > 0 && (!x || !u)) return fail(CRX_ERR_ARG, "NULL array argument");
    if (n_groups > 0 && ws_bytes < crx_sysid_workspace_bytes(d, n_logs, n_groups, max_log_rows))
        return fail(CRX_ERR_ARG, "workspace of %zu bytes, %zu needed", ws_bytes, crx_sysid_workspace_bytes(d, n_logs, n_groups, max_log_rows));
    if (((uintptr_t)x | (uintptr_t)u) & 15) return fail(CRX_ERR_ARG, "x and u must be 16-byte aligned");
    if (int rc = ensure_init()) return rc;
    if (n_groups == 0) return CRX_OK;
    crx_sysid_kparams kp;
    kp.n_logs = n_logs; kp.n_groups = n_groups; kp.first_row = d->first_row; kp.chunk = d->chunk_rows; kp.tpl = tpl; kp.lamb = d->lamb;
    kp.log_off = log_offset; kp.grp_off = group_offset; kp.x = x; kp.u = u;
    char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    const size_t tiles = (size_t)n_logs * tpl;
    kp.ws_gram = (double*)ws;
    kp.ws_res = kp.ws_gram + tiles * 84;
    kp.ws_W = kp.ws_res + tiles * 12;
    kp.A = A; kp.B = B; kp.err = err; kp.n_pairs = n_pairs; kp.status = status;
    return launched(crx_launch_sysid(kp, (hipStream_t)stream), "sysid");
}

int crx_sysid_fit(const crx_sysid_desc* d, int n_logs, const int64_t* log_offset, const int32_t* group_offset, int n_groups,
                  const double* x, const double* u, double* A, double* B, double* err, int64_t* n_pairs, int32_t* status) {
    if (int rc = check_sysid(d, n_logs, log_offset, group_offset, n_groups, 0, A, B, err, n_pairs, status)) return rc;
    int64_t max_rows = 0, rows = 0;
    if (n_groups > 0) {
        if (log_offset[0] < 0) return fail(CRX_ERR_ARG, "log_offset[0] < 0");
        for (int l = 0; l < n_logs; l++) {
            const int64_t n = log_offset[l + 1] - log_offset[l];
            if (n < 0) return fail(CRX_ERR_ARG, "log_offset decreases at %d", l);
            if (n > max_rows) max_rows = n;
        }
        rows = log_offset[n_logs];
        if (group_offset) {
            if (group_offset[0] != 0 || group_offset[n_groups] != n_logs) return fail(CRX_ERR_ARG, "group_offset must run from 0 to n_logs");
            for (int g = 0; g < n_groups; g++)
                if (group_offset[g + 1] < group_offset[g]) return fail(CRX_ERR_ARG, "group_offset decreases at %d", g);
        }
        if (rows > 0 && (!x || !u)) return fail(CRX_ERR_ARG, "NULL array argument");
    }
    if (int rc = ensure_init()) return rc;
    if (n_groups == 0) return CRX_OK;
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    const size_t L = (size_t)n_logs, G = (size_t)n_groups, R = (size_t)rows;
    const size_t ws_bytes = crx_sysid_workspace_bytes(d, n_logs, n_groups, max_rows);
    Stage sg;
    auto dx = sg.in(x, R * 6); auto du = sg.in(u, R * 2); auto dlo = sg.in(log_offset, L + 1);
    auto dgo = group_offset ? sg.in(group_offset, G + 1) : Stage::Ref<int32_t>{};
    auto dA = sg.out(A, G * 36); auto dB = sg.out(B, G * 12); auto de = sg.out(err, G * 12);
    auto dn = sg.out(n_pairs, G); auto ds = sg.out(status, G);
    auto dws = sg.scratch(ws_bytes);   // the tile partials stay on the device: the copy back stops in front of them
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_sysid_fit_dev(d, n_logs, sg[dlo], sg[dgo], n_groups, max_rows, sg[dx], sg[du], sg[dws], ws_bytes, sg[dA], sg[dB], sg[de],
                                   sg[dn], sg[ds], g_stream)) return rc;
    return sg.down(g_stream);
}

// ---- PID step + log row of the identification experiment (control/control.py:15-25, utils/base.py PIDTracking) ------------
int crx_pid_log_dev(int batch, int T, int row, const double* vt, const double* eyt, const double* xcurv, const double* u_prev,
                    double* u_next, double* x_log, double* u_log, void* stream) {
    if (batch < 0 || row >= T) return fail(CRX_ERR_ARG, "batch < 0 or row >= T");
    if (batch > 0 && (!xcurv || (u_next && (!vt || !eyt)) || (row >= 0 && (!u_prev || !x_log || !u_log))))
        return fail(CRX_ERR_ARG, "NULL array argument");
    if (int rc = ensure_init()) return rc;
    if (batch == 0) return CRX_OK;
    crx_pid_kparams kp;
    kp.batch = batch; kp.T = T; kp.row = row; kp.vt = vt; kp.eyt = eyt; kp.xcurv = xcurv; kp.u_prev = u_prev;
    kp.u_next = u_next; kp.x_log = x_log; kp.u_log = u_log;
    return launched(crx_launch_pid_log(kp, (hipStream_t)stream), "pid");
}

// ---- planner front (interest test, partial sort, vehicle infos) on the device ------------------------
void crx_scene_desc_default(crx_scene_desc* d, int N, int n_all_max, int n_veh_max, double lap_length) {
    memset(d, 0, sizeof(*d));
    d->N = N; d->n_all_max = n_all_max; d->n_veh_max = n_veh_max;
    d->safety_factor = 4.5; d->prediction_factor = 0.5; d->veh_length = 0.4; d->lap_length = lap_length;
}

static int check_scene(const crx_scene_desc* d, int n_scen, arr ego_xcurv, arr n_all, arr veh_xcurv, arr pred_s, arr pred_ey, arr n_veh, arr overflow,
                       arr order, arr veh_info, arr max_dv, arr obs_s, arr obs_ey) {
    if (int rc = ensure_init()) return rc;
    if (!d) return fail(CRX_ERR_ARG, "desc is NULL");
    if (d->N < 1 || d->N > CRX_MAX_N) return fail(CRX_ERR_ARG, "N=%d outside [1,%d]", d->N, CRX_MAX_N);
    if (d->n_all_max < 1 || d->n_all_max > 64) return fail(CRX_ERR_ARG, "n_all_max=%d outside [1,64]", d->n_all_max);
    if (d->n_veh_max < 1 || d->n_veh_max > CRX_MAX_VEH) return fail(CRX_ERR_ARG, "n_veh_max=%d outside [1,%d]", d->n_veh_max, CRX_MAX_VEH);
    if (!(d->lap_length > 0.0) || !isfinite(d->lap_length)) return fail(CRX_ERR_ARG, "lap_length must be positive and finite");
    if (n_scen < 0) return fail(CRX_ERR_ARG, "n_scen < 0");
    if (n_scen > 0 && any_null(ego_xcurv, n_all, veh_xcurv, pred_s, pred_ey, n_veh, overflow, order, veh_info, max_dv, obs_s, obs_ey))
        return fail(CRX_ERR_ARG, "NULL array argument");
    return 0;
}

int crx_planner_scene_dev(const crx_scene_desc* d, int n_scen, const double* ego_xcurv, const int32_t* n_all,
                          const double* veh_xcurv, const double* pred_s, const double* pred_ey, int32_t* n_veh,
                          int32_t* overflow, int32_t* order, double* veh_info, double* max_dv, double* obs_s, double* obs_ey,
                          void* stream) {
    if (int rc = check_scene(d, n_scen, ego_xcurv, n_all, veh_xcurv, pred_s, pred_ey, n_veh, overflow, order, veh_info, max_dv, obs_s, obs_ey))
        return rc;
    if (n_scen == 0) return CRX_OK;
    crx_scene_kparams sp;
    sp.d = *d; sp.n_scen = n_scen; sp.ego_xcurv = ego_xcurv; sp.n_all = n_all; sp.veh_xcurv = veh_xcurv; sp.pred_s = pred_s;
    sp.pred_ey = pred_ey; sp.n_veh = n_veh; sp.overflow = overflow; sp.order = order; sp.veh_info = veh_info; sp.max_dv = max_dv;
    sp.obs_s = obs_s; sp.obs_ey = obs_ey;
    return launched(crx_launch_scene(sp, (hipStream_t)stream), "scene");
}

int crx_planner_scene(const crx_scene_desc* d, int n_scen, const double* ego_xcurv, const int32_t* n_all, const double* veh_xcurv,
                      const double* pred_s, const double* pred_ey, int32_t* n_veh, int32_t* overflow, int32_t* order,
                      double* veh_info, double* max_dv, double* obs_s, double* obs_ey) {
    if (int rc = check_scene(d, n_scen, ego_xcurv, n_all, veh_xcurv, pred_s, pred_ey, n_veh, overflow, order, veh_info, max_dv, obs_s, obs_ey))
        return rc;
    if (n_scen == 0) return CRX_OK;
    for (int i = 0; i < n_scen; i++)
        if (n_all[i] < 0 || n_all[i] > d->n_all_max) return fail(CRX_ERR_ARG, "n_all[%d]=%d outside [0,%d]", i, n_all[i], d->n_all_max);
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    const size_t S = (size_t)n_scen, VA = (size_t)d->n_all_max, V = (size_t)d->n_veh_max, N1 = (size_t)d->N + 1;
    Stage sg;
    auto dego = sg.in(ego_xcurv, S * 6); auto dvx = sg.in(veh_xcurv, S * VA * 6);
    auto dps = sg.in(pred_s, S * VA * N1); auto dpe = sg.in(pred_ey, S * VA * N1); auto dna = sg.in(n_all, S);
    auto dnv = sg.out(n_veh, S); auto dov = sg.out(overflow, S); auto dor = sg.out(order, S * V);
    auto dvi = sg.out(veh_info, S * V * 3); auto dmd = sg.out(max_dv, S);
    auto dos = sg.out(obs_s, S * V * N1); auto doe = sg.out(obs_ey, S * V * N1);
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_planner_scene_dev(d, n_scen, sg[dego], sg[dna], sg[dvx], sg[dps], sg[dpe], sg[dnv], sg[dov], sg[dor], sg[dvi], sg[dmd],
                                       sg[dos], sg[doe], g_stream)) return rc;
    return sg.down(g_stream);
}

// ---- inputs of the tracking NLP from the planner's outputs, on the device ----------------------------
int crx_track_prep_dev(int N, int V, double lap_length, double safety_time, double dt_ref, int batch, const double* x,
                       const int32_t* n_veh, const double* obs_s_in, const double* obs_ey_in, const double* traj, double* xt,
                       double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs, void* stream) {
    if (int rc = ensure_init()) return rc;
    if (N < 1 || N > CRX_MAX_N || V < 1 || V > CRX_MAX_OBS || batch < 0 || !(lap_length > 0.0) || !isfinite(lap_length))
        return fail(CRX_ERR_ARG, "bad track prep dimensions");
    if (batch == 0) return CRX_OK;
    if (!x || !n_veh || !obs_s_in || !obs_ey_in || !traj || !xt || !obs_s || !obs_ey || !lap_off || !n_obs) return fail(CRX_ERR_ARG, "NULL array argument");
    crx_trackprep_kparams tp;
    tp.N = N; tp.V = V; tp.batch = batch; tp.lap_length = lap_length; tp.safety_time = safety_time; tp.dt_ref = dt_ref;
    tp.x = x; tp.n_veh = n_veh; tp.obs_s_in = obs_s_in; tp.obs_ey_in = obs_ey_in; tp.traj = traj;
    tp.xt = xt; tp.obs_s = obs_s; tp.obs_ey = obs_ey; tp.lap_off = lap_off; tp.n_obs = n_obs;
    return launched(crx_launch_trackprep(tp, (hipStream_t)stream), "track prep");
}

// ---- learning-MPC host prep on the device ------------------------------------------------------------
void crx_lmpcprep_desc_default(crx_lmpcprep_desc* d, int N, int n_points, int n_laps, int n_seg, double dt, double lap_length) {
    memset(d, 0, sizeof(*d));
    d->N = N; d->n_points = n_points; d->n_laps = n_laps; d->n_ss_per_lap = 22; d->n_ss_laps = 2; d->max_neighbours = 40;
    d->n_seg = n_seg; d->shift = 0; d->bandwidth = 5.0;
    d->scale[0] = 0.1; d->scale[1] = d->scale[2] = d->scale[3] = d->scale[4] = 1.0;
    d->dt = dt; d->lap_length = lap_length;
}

static int check_lmpcprep(const crx_lmpcprep_desc* d, int batch) {
    if (!d) return fail(CRX_ERR_ARG, "desc is NULL");
    if (d->N < 2 || d->N > CRX_LMPC_MAX_N) return fail(CRX_ERR_ARG, "N=%d outside [2,%d]", d->N, CRX_LMPC_MAX_N);
    if (d->n_points < 2 || d->n_points > 65535 || d->n_laps < 2) return fail(CRX_ERR_ARG, "n_points outside [2,65535] or n_laps < 2");
    if (d->n_ss_laps < 1 || d->n_ss_laps > 2 || d->n_ss_per_lap < 1 || d->n_ss_laps * d->n_ss_per_lap > CRX_MAX_SS)
        return fail(CRX_ERR_ARG, "n_ss_laps outside [1,2] or more than %d safe-set points", CRX_MAX_SS);
    if (d->max_neighbours < 1 || d->max_neighbours > 64) return fail(CRX_ERR_ARG, "max_neighbours outside [1,64]");
    if (d->n_seg < 1 || !(d->bandwidth > 0.0) || !(d->dt > 0.0) || !(d->lap_length > 0.0) || !isfinite(d->lap_length))
        return fail(CRX_ERR_ARG, "n_seg, bandwidth, dt and lap_length must be positive");
    if (batch < 0) return fail(CRX_ERR_ARG, "batch < 0");
    if (crx_lmpcprep_lds_bytes(d->n_points) > 160 * 1024) return fail(CRX_ERR_ARG, "n_points=%d needs more than 160 KiB of LDS", d->n_points);
    return 0;
}

static int check_lmpcprep_call(const crx_lmpcprep_desc* d, int batch, arr ss_xcurv, arr u_ss, arr qfun, arr time_ss, arr iter, arr x, arr lin_points,
                               arr lin_input, arr track, arr A, arr B, arr C, arr ss_sel, arr q_sel, arr status) {
    if (int rc = ensure_init()) return rc;
    if (int rc = check_lmpcprep(d, batch)) return rc;
    if (batch > 0 && any_null(ss_xcurv, u_ss, qfun, time_ss, iter, x, lin_points, lin_input, track, A, B, C, ss_sel, q_sel, status))
        return fail(CRX_ERR_ARG, "NULL array argument");
    return 0;
}

int crx_lmpc_prep_dev(const crx_lmpcprep_desc* d, int batch, const double* ss_xcurv, const double* u_ss, const double* qfun,
                      const int32_t* time_ss, const int32_t* iter, const double* x, const double* lin_points,
                      const double* lin_input, int from_plan, const double* track, double* A, double* B, double* C,
                      double* ss_sel, double* q_sel, int32_t* status, void* stream) {
    return crx_lmpc_prep_masked_dev(d, batch, nullptr, ss_xcurv, u_ss, qfun, time_ss, iter, x, lin_points, lin_input, from_plan, track, A, B, C,
                                    ss_sel, q_sel, status, stream);
}

int crx_lmpc_prep_masked_dev(const crx_lmpcprep_desc* d, int batch, const int32_t* active, const double* ss_xcurv, const double* u_ss,
                             const double* qfun, const int32_t* time_ss, const int32_t* iter, const double* x, const double* lin_points,
                             const double* lin_input, int from_plan, const double* track, double* A, double* B, double* C,
                             double* ss_sel, double* q_sel, int32_t* status, void* stream) {
    if (int rc = check_lmpcprep_call(d, batch, ss_xcurv, u_ss, qfun, time_ss, iter, x, lin_points, lin_input, track, A, B, C, ss_sel, q_sel,
                                     status)) return rc;
    if (batch == 0) return CRX_OK;
    crx_lmpcprep_kparams kp;
    kp.d = *d; kp.batch = batch; kp.from_plan = from_plan ? 1 : 0;
    kp.ss_xcurv = ss_xcurv; kp.u_ss = u_ss; kp.qfun = qfun; kp.time_ss = time_ss; kp.iter = iter; kp.x = x;
    kp.lin_points = lin_points; kp.lin_input = lin_input; kp.track = track;
    kp.A = A; kp.B = B; kp.C = C; kp.ss_sel = ss_sel; kp.q_sel = q_sel; kp.status = status; kp.active = active;
    return launched(crx_launch_lmpcprep(kp, (hipStream_t)stream), "lmpc prep");
}

int crx_lmpc_prep(const crx_lmpcprep_desc* d, int batch, const double* ss_xcurv, const double* u_ss, const double* qfun,
                  const int32_t* time_ss, const int32_t* iter, const double* x, const double* lin_points,
                  const double* lin_input, int from_plan, const double* track, double* A, double* B, double* C,
                  double* ss_sel, double* q_sel, int32_t* status) {
    if (int rc = check_lmpcprep_call(d, batch, ss_xcurv, u_ss, qfun, time_ss, iter, x, lin_points, lin_input, track, A, B, C, ss_sel, q_sel,
                                     status)) return rc;
    if (batch == 0) return CRX_OK;
    const size_t Bn = (size_t)batch, N = (size_t)d->N, P = (size_t)d->n_points, L = (size_t)d->n_laps;
    const size_t M = (size_t)d->n_ss_per_lap * d->n_ss_laps;
    for (size_t b = 0; b < Bn; b++) {
        if (iter[b] < 2 || iter[b] > (int)L) return fail(CRX_ERR_ARG, "iter[%zu]=%d outside [2,%zu]", b, iter[b], L);
        for (int k = 0; k < 2; k++) {
            const int t = time_ss[b * L + iter[b] - 2 + k];
            if (t < 2 || t > (int)P) return fail(CRX_ERR_ARG, "time_ss of a lap used by race %zu is %d, outside [2,%zu]", b, t, P);
        }
    }
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    Stage sg;
    auto dss = sg.in(ss_xcurv, Bn * L * P * 6); auto dus = sg.in(u_ss, Bn * L * P * 2); auto dqf = sg.in(qfun, Bn * L * P);
    auto dx = sg.in(x, Bn * 6); auto dlp = sg.in(lin_points, Bn * (N + 1) * 6); auto dli = sg.in(lin_input, Bn * N * 2);
    auto dtr = sg.in(track, (size_t)d->n_seg * 6);
    auto dts = sg.in(time_ss, Bn * L); auto dit = sg.in(iter, Bn);
    // A, B, C are in/out: a singular stage leaves its three regression rows untouched (include/crx.h), so the staging copies
    // start from the caller's arrays, not from whatever an earlier call left in the staging buffer
    auto dA = sg.inout(A, Bn * N * 36); auto dB = sg.inout(B, Bn * N * 12); auto dC = sg.inout(C, Bn * N * 6);
    auto dsel = sg.out(ss_sel, Bn * 6 * M); auto dq = sg.out(q_sel, Bn * M); auto dst = sg.out(status, Bn);
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_lmpc_prep_dev(d, batch, sg[dss], sg[dus], sg[dqf], sg[dts], sg[dit], sg[dx], sg[dlp], sg[dli], from_plan, sg[dtr], sg[dA],
                                   sg[dB], sg[dC], sg[dsel], sg[dq], sg[dst], g_stream)) return rc;
    return sg.down(g_stream);
}

int crx_lmpc_addpoint_dev(const crx_lmpcprep_desc* d, int batch, double* ss_xcurv, double* u_ss, const int32_t* time_ss,
                          const int32_t* iter, const int32_t* step, const double* x, const double* u, int u_stride, void* stream) {
    if (int rc = ensure_init()) return rc;
    if (int rc = check_lmpcprep(d, batch)) return rc;
    if (u_stride < 2) return fail(CRX_ERR_ARG, "u_stride < 2");
    if (batch == 0) return CRX_OK;
    if (!ss_xcurv || !u_ss || !time_ss || !iter || !step || !x || !u) return fail(CRX_ERR_ARG, "NULL array argument");
    return launched(crx_launch_lmpc_addpoint(*d, batch, ss_xcurv, u_ss, time_ss, iter, step, x, u, u_stride, (hipStream_t)stream), "lmpc addpoint");
}

int crx_lmpc_addtraj_dev(const crx_lmpcprep_desc* d, int batch, const int32_t* crossed, double* log_x, const double* log_u,
                         int32_t* n_log, double* ss_xcurv, double* u_ss, double* qfun, int32_t* time_ss, int32_t* iter,
                         int32_t* step, const double* x, int32_t* status, void* stream) {
    if (int rc = ensure_init()) return rc;
    if (int rc = check_lmpcprep(d, batch)) return rc;
    if (batch == 0) return CRX_OK;
    if (!crossed || !log_x || !log_u || !n_log || !ss_xcurv || !u_ss || !qfun || !time_ss || !iter || !step || !x || !status)
        return fail(CRX_ERR_ARG, "NULL array argument");
    return launched(crx_launch_lmpc_addtraj(*d, batch, crossed, log_x, log_u, n_log, ss_xcurv, u_ss, qfun, time_ss, iter, step, x, status,
                                           (hipStream_t)stream), "lmpc addtraj");
}

// ---- fused planner step ------------------------------------------------------------------------------
// the two descriptors of the fused step are looked at before the device is (unlike every family above)
static int check_plan_descs(const crx_planner_desc* d, const crx_select_desc* sd) {
    if (!d || !sd) return fail(CRX_ERR_ARG, "desc is NULL");
    if (sd->N != d->N) return fail(CRX_ERR_ARG, "planner and selection horizons differ");
    return 0;
}

int crx_planner_plan_dev(const crx_planner_desc* d, const crx_select_desc* sd, int n_scen, const double* x0,
                         const double* bez_s, const double* bez_ey, const double* ey_lb, const double* ey_ub,
                         const int32_t* n_veh, const double* obs_s, const double* obs_ey, const int32_t* old_flag,
                         double* X, double* U, double* cost, int32_t* status, double* kkt, int32_t* iters,
                         int32_t* flag, double* sel_cost, double* best_X, void* stream) {
    return crx_planner_plan_masked_dev(d, sd, n_scen, nullptr, x0, bez_s, bez_ey, ey_lb, ey_ub, n_veh, obs_s, obs_ey, old_flag, X, U, cost,
                                       status, kkt, iters, flag, sel_cost, best_X, stream);
}

int crx_planner_plan_masked_dev(const crx_planner_desc* d, const crx_select_desc* sd, int n_scen, const int32_t* active,
                                const double* x0, const double* bez_s, const double* bez_ey, const double* ey_lb,
                                const double* ey_ub, const int32_t* n_veh, const double* obs_s, const double* obs_ey,
                                const int32_t* old_flag, double* X, double* U, double* cost, int32_t* status, double* kkt,
                                int32_t* iters, int32_t* flag, double* sel_cost, double* best_X, void* stream) {
    return crx_planner_plan_models_dev(d, sd, n_scen, active, x0, nullptr, nullptr, nullptr, bez_s, bez_ey, ey_lb, ey_ub, n_veh, obs_s, obs_ey,
                                       old_flag, X, U, cost, status, kkt, iters, flag, sel_cost, best_X, stream);
}

// (the models are the region QPs': one per problem, [n_scen * (n_veh_max + 1)], indexed like x0)
int crx_planner_plan_models_dev(const crx_planner_desc* d, const crx_select_desc* sd, int n_scen, const int32_t* active,
                                const double* x0, const double* model_A, const double* model_B, const double* model_reach,
                                const double* bez_s, const double* bez_ey, const double* ey_lb, const double* ey_ub,
                                const int32_t* n_veh, const double* obs_s, const double* obs_ey, const int32_t* old_flag, double* X,
                                double* U, double* cost, int32_t* status, double* kkt, int32_t* iters, int32_t* flag, double* sel_cost,
                                double* best_X, void* stream) {
    if (int rc = check_plan_descs(d, sd)) return rc;
    if (int rc = check_select(sd, n_scen)) return rc;   // before R = n_veh_max + 1 sizes the QP launch
    const int R = sd->n_veh_max + 1;
    if ((long long)n_scen * R > 0x7fffffffLL) return fail(CRX_ERR_ARG, "n_scen * (n_veh_max + 1) overflows int");
    if (int rc = planner_solve_masked(d, n_scen * R, active, R, x0, model_A, model_B, model_reach, bez_s, bez_ey, ey_lb, ey_ub, X, U, cost, status,
                                      kkt, iters, stream)) return rc;
    return crx_select_dev(sd, n_scen, n_veh, X, obs_s, obs_ey, old_flag, flag, sel_cost, best_X, stream);
}

int crx_planner_plan(const crx_planner_desc* d, const crx_select_desc* sd, int n_scen, const double* x0,
                     const double* bez_s, const double* bez_ey, const double* ey_lb, const double* ey_ub,
                     const int32_t* n_veh, const double* obs_s, const double* obs_ey, const int32_t* old_flag,
                     double* X, double* U, double* cost, int32_t* status, double* kkt, int32_t* iters,
                     int32_t* flag, double* sel_cost, double* best_X) {
    return crx_planner_plan_models(d, sd, n_scen, x0, nullptr, nullptr, bez_s, bez_ey, ey_lb, ey_ub, n_veh, obs_s, obs_ey, old_flag, X, U, cost,
                                   status, kkt, iters, flag, sel_cost, best_X);
}

int crx_planner_plan_models(const crx_planner_desc* d, const crx_select_desc* sd, int n_scen, const double* x0, const double* model_A,
                            const double* model_B, const double* bez_s, const double* bez_ey, const double* ey_lb,
                            const double* ey_ub, const int32_t* n_veh, const double* obs_s, const double* obs_ey,
                            const int32_t* old_flag, double* X, double* U, double* cost, int32_t* status, double* kkt, int32_t* iters,
                            int32_t* flag, double* sel_cost, double* best_X) {
    if (int rc = check_plan_descs(d, sd)) return rc;
    if (n_scen < 0) return fail(CRX_ERR_ARG, "n_scen < 0");
    if (int rc = check_planner_models((model_A != nullptr) + (model_B != nullptr), 2)) return rc;
    if (int rc = ensure_init()) return rc;
    crx_kparams chk;
    const bool models = model_A || model_B;
    if (int rc = fill_planner(chk, d, 0, !models)) return rc;
    if (int rc = check_select(sd, n_scen)) return rc;
    if (n_scen == 0) return CRX_OK;
    if (planner_null(x0, bez_s, bez_ey, ey_lb, ey_ub, X, U, cost, status, kkt, iters) ||
        select_null(sd, n_veh, X, obs_s, obs_ey, old_flag, flag, sel_cost, best_X))
        return fail(CRX_ERR_ARG, "NULL array argument");
    const size_t S = (size_t)n_scen, N = (size_t)d->N, V = (size_t)sd->n_veh_max, R = V + 1, B = S * R;
    for (size_t i = 0; i < S; i++)
        if (n_veh[i] < 0 || n_veh[i] > (int)V) return fail(CRX_ERR_ARG, "n_veh[%zu]=%d outside [0,%zu]", i, n_veh[i], V);
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    // one staging round trip for the whole step; X stays on the device between the two kernels
    Stage sg;
    auto dx0 = sg.in(x0, B * 6); auto dbs = sg.in(bez_s, B * (N + 1)); auto dbe = sg.in(bez_ey, B * (N + 1));
    auto dlb = sg.in(ey_lb, B * N); auto dub = sg.in(ey_ub, B);
    auto dos = sg.in(obs_s, S * V * (N + 1)); auto doe = sg.in(obs_ey, S * V * (N + 1));
    auto dnv = sg.in(n_veh, S); auto dof = sg.in(old_flag, S);
    auto dmA = models ? sg.in(model_A, B * 36) : Stage::Ref<double>{};
    auto dmB = models ? sg.in(model_B, B * 12) : Stage::Ref<double>{};
    auto dmR = models ? sg.scratch(CRX_PLANNER_MODEL_REACH_DOUBLES(B) * sizeof(double)) : Stage::Ref<char>{};
    auto dX = sg.out(X, B * (N + 1) * 6); auto dU = sg.out(U, B * N * 2); auto dc = sg.out(cost, B); auto dk = sg.out(kkt, B);
    auto ds = sg.out(status, B); auto di = sg.out(iters, B);
    auto dfl = sg.out(flag, S); auto dsc = sg.out(sel_cost, S * R); auto dbX = sg.out(best_X, S * (N + 1) * 6);
    if (int rc = sg.up(g_stream)) return rc;
    if (models)
        if (int rc = crx_planner_models_reach_dev(d, (int)B, sg[dmA], sg[dmB], (double*)sg[dmR], g_stream)) return rc;
    if (int rc = crx_planner_plan_models_dev(d, sd, n_scen, nullptr, sg[dx0], sg[dmA], sg[dmB], (double*)sg[dmR], sg[dbs], sg[dbe], sg[dlb], sg[dub],
                                             sg[dnv], sg[dos], sg[doe], sg[dof], sg[dX], sg[dU], sg[dc], sg[ds], sg[dk], sg[di], sg[dfl], sg[dsc],
                                             sg[dbX], g_stream)) return rc;
    return sg.down(g_stream);
}

}  // extern "C"

// ---- dispatch order of a solver launch ------------------------------------------------------------------------------
extern "C" {

int crx_order_longest_first_dev(int batch, const int32_t* iters, const int32_t* active, int32_t* order, void* stream) {
    if (int rc = ensure_init()) return rc;
    if (batch < 0) return fail(CRX_ERR_ARG, "bad batch");
    if (batch == 0) return CRX_OK;
    if (!iters || !order) return fail(CRX_ERR_ARG, "NULL array argument");
    crx_order_kparams op;
    memset(&op, 0, sizeof(op));
    op.batch = batch; op.mode = 0; op.iters = iters; op.active = active; op.order = order;
    return launched(crx_launch_order(op, (hipStream_t)stream), "order");
}

int crx_cbf_order_dev(const crx_cbf_desc* d, int batch, const int32_t* active, const double* x0, const double* xt,
                      const double* obs_s, const double* obs_ey, const double* lap_off, const int32_t* n_obs, const double* obs_dims,
                      int32_t* order, void* stream) {
    if (int rc = ensure_init()) return rc;
    if (!d || batch < 0) return fail(CRX_ERR_ARG, "bad descriptor / batch");
    if (d->N < 1 || d->N > CRX_MAX_N || d->n_obs_max < 0 || d->n_obs_max > CRX_MAX_OBS) return fail(CRX_ERR_ARG, "bad N / n_obs_max");
    if (d->degree != 2 && d->degree != 4 && d->degree != 6 && d->degree != 8) return fail(CRX_ERR_ARG, "degree must be 2, 4, 6 or 8");
    if (batch == 0) return CRX_OK;
    if (!x0 || !xt || !order || (d->n_obs_max > 0 && (!obs_s || !obs_ey || !lap_off || !n_obs))) return fail(CRX_ERR_ARG, "NULL array argument");
    crx_order_kparams op;
    memset(&op, 0, sizeof(op));
    op.batch = batch; op.mode = 1; op.active = active; op.order = order;
    op.V = d->n_obs_max; op.stride = d->N + 1; op.degree = d->degree; op.margin = d->margin; op.l_sum = d->l_sum; op.w_sum = d->w_sum;
    op.per_stage_target = d->per_stage_target; op.ds_per_vx = d->A[4 * 6 + 0]; op.xt = xt;
    op.x0 = x0; op.obs_s = obs_s; op.obs_ey = obs_ey; op.lap_off = lap_off; op.obs_dims = d->n_obs_max > 0 ? obs_dims : nullptr; op.n_obs = n_obs;
    return launched(crx_launch_order(op, (hipStream_t)stream), "order");
}

}  // extern "C"

// ---- device-resident racing-game loop: bookkeeping between the solver launches ----------------------------------
extern "C" {

int crx_game_traffic_dev(int N, int batch, int n_cars, double lap_length, double t, double dt, const double* car_s0, const double* car_v,
                         const double* car_ey, double* veh_xcurv, double* pred_s, double* pred_ey, void* stream) {
    if (int rc = ensure_init()) return rc;
    if (N < 1 || N > CRX_MAX_N || batch < 0 || n_cars < 0 || !(lap_length > 0.0)) return fail(CRX_ERR_ARG, "bad game traffic dimensions");
    if (batch == 0 || n_cars == 0) return CRX_OK;
    if (!car_s0 || !car_v || !car_ey || !veh_xcurv || !pred_s || !pred_ey) return fail(CRX_ERR_ARG, "NULL array argument");
    crx_game_kparams gp;
    memset(&gp, 0, sizeof(gp));
    gp.Np = N; gp.batch = batch; gp.n_cars = n_cars; gp.lap_length = lap_length; gp.t = t; gp.dt = dt;
    gp.car_s0 = car_s0; gp.car_v = car_v; gp.car_ey = car_ey; gp.veh_xcurv = veh_xcurv; gp.pred_s = pred_s; gp.pred_ey = pred_ey;
    return launched(crx_launch_game(0, gp, (hipStream_t)stream), "game traffic");
}

int crx_game_masks_dev(int batch, const int32_t* n_veh, const int32_t* overflow, int32_t* m_overtake, int32_t* m_lmpc,
                       int32_t* overflow_seen, void* stream) {
    if (int rc = ensure_init()) return rc;
    if (batch < 0) return fail(CRX_ERR_ARG, "batch < 0");
    if (batch == 0) return CRX_OK;
    if (!n_veh || !m_overtake || !m_lmpc) return fail(CRX_ERR_ARG, "NULL array argument");
    crx_game_kparams gp;
    memset(&gp, 0, sizeof(gp));
    gp.batch = batch; gp.n_veh = n_veh; gp.m_overtake = m_overtake; gp.m_lmpc = m_lmpc;
    if (overflow && overflow_seen) { gp.overflow = overflow; gp.overflow_seen = overflow_seen; }
    return launched(crx_launch_game(1, gp, (hipStream_t)stream), "game masks");
}

int crx_game_commit_dev(int N, int Np, int batch, const int32_t* overtake, const double* U_track, const double* X_lmpc,
                        const double* U_lmpc, const int32_t* flag, double* u, double* u_old, double* u_prev, double* lin_points,
                        double* lin_input, int32_t* step_no, int32_t* addpoint_step, int32_t* old_flag, void* stream) {
    if (int rc = ensure_init()) return rc;
    if (N < 1 || N > CRX_MAX_N || batch < 0 || (overtake && (Np < 1 || Np > CRX_MAX_N))) return fail(CRX_ERR_ARG, "bad game commit dimensions");
    if (batch == 0) return CRX_OK;
    if (!X_lmpc || !U_lmpc || !u || !u_old || !u_prev || !lin_points || !lin_input || !step_no || !addpoint_step)
        return fail(CRX_ERR_ARG, "NULL array argument");
    if (overtake && (!U_track || (old_flag && !flag))) return fail(CRX_ERR_ARG, "NULL overtake-branch array");
    crx_game_kparams gp;
    memset(&gp, 0, sizeof(gp));
    gp.N = N; gp.Np = Np; gp.batch = batch; gp.overtake = overtake; gp.U_track = U_track; gp.X_lmpc = X_lmpc; gp.U_lmpc = U_lmpc;
    gp.flag = flag; gp.u = u; gp.u_old = u_old; gp.u_prev = u_prev; gp.lin_points = lin_points; gp.lin_input = lin_input;
    gp.step_no = step_no; gp.addpoint_step = addpoint_step; gp.old_flag = old_flag;
    return launched(crx_launch_game(2, gp, (hipStream_t)stream), "game commit");
}

int crx_game_log_dev(int batch, int n_points, double lap_length, const double* xcurv, const double* u, const int32_t* laps,
                     int32_t* laps_prev, double* log_x, double* log_u, int32_t* n_log, int32_t* crossed, void* stream) {
    if (int rc = ensure_init()) return rc;
    if (batch < 0 || n_points < 2) return fail(CRX_ERR_ARG, "bad game log dimensions");
    if (batch == 0) return CRX_OK;
    if (!xcurv || !u || !laps || !laps_prev || !log_x || !log_u || !n_log || !crossed) return fail(CRX_ERR_ARG, "NULL array argument");
    crx_game_kparams gp;
    memset(&gp, 0, sizeof(gp));
    gp.batch = batch; gp.n_points = n_points; gp.lap_length = lap_length; gp.xcurv = xcurv; gp.u = (double*)u; gp.laps = laps;
    gp.laps_prev = laps_prev; gp.log_x = log_x; gp.log_u = log_u; gp.n_log = n_log; gp.crossed = crossed;
    return launched(crx_launch_game(3, gp, (hipStream_t)stream), "game log");
}

// seed laps (include/crx.h S1-S6): device-pointer entries only, like the rest of the family
int crx_seed_commit_dev(int N, int batch, const int32_t* phase, const double* vt, const double* eyt, const double* x, const double* U_mpc,
                        const int32_t* mpc_status, int32_t* seed_status, double* u, void* stream) {
    if (int rc = ensure_init()) return rc;
    if (N < 1 || N > CRX_MAX_N || batch < 0) return fail(CRX_ERR_ARG, "bad seed commit dimensions");
    if (batch == 0) return CRX_OK;
    if (!phase || !vt || !eyt || !x || !U_mpc || !mpc_status || !seed_status || !u) return fail(CRX_ERR_ARG, "NULL array argument");
    crx_seed_kparams sp;
    memset(&sp, 0, sizeof(sp));
    sp.batch = batch; sp.u_stride = 2 * N; sp.phase = (int32_t*)phase; sp.vt = vt; sp.eyt = eyt; sp.x = x; sp.U_mpc = U_mpc;
    sp.mpc_status = mpc_status; sp.seed_status = seed_status; sp.u = u;
    return launched(crx_launch_seed(0, sp, (hipStream_t)stream), "seed commit");
}

int crx_seed_log_dev(int batch, int n_points, double lap_length, const double* xcurv_prev, const double* xglob_prev, double* xcurv,
                     double* xglob, const double* u, int32_t* laps, int32_t* laps_prev, double* log_x, double* log_u, int32_t* n_log,
                     int32_t* crossed, int32_t* phase, int32_t* seed_status, int32_t* m_mpc, void* stream) {
    if (int rc = ensure_init()) return rc;
    if (batch < 0 || n_points < 2) return fail(CRX_ERR_ARG, "bad seed log dimensions");
    if (batch == 0) return CRX_OK;
    if (!xcurv_prev || !xglob_prev || !xcurv || !xglob || !u || !laps || !laps_prev || !log_x || !log_u || !n_log || !crossed || !phase ||
        !seed_status || !m_mpc)
        return fail(CRX_ERR_ARG, "NULL array argument");
    if (xcurv_prev == xcurv || xglob_prev == xglob) return fail(CRX_ERR_ARG, "the plant's two state pairs must be different arrays");
    crx_seed_kparams sp;
    memset(&sp, 0, sizeof(sp));
    sp.batch = batch; sp.n_points = n_points; sp.lap_length = lap_length; sp.xcurv_prev = xcurv_prev; sp.xglob_prev = xglob_prev;
    sp.xcurv = xcurv; sp.xglob = xglob; sp.u = (double*)u; sp.laps = laps; sp.laps_prev = laps_prev; sp.log_x = log_x; sp.log_u = log_u;
    sp.n_log = n_log; sp.crossed = crossed; sp.phase = phase; sp.seed_status = seed_status; sp.m_mpc = m_mpc;
    return launched(crx_launch_seed(1, sp, (hipStream_t)stream), "seed log");
}

}  // extern "C"

// ---- race statistics: per-car outcomes of every closed loop (crx_race_stats_*_kernel, crx_game.hip) -------------------------------
extern "C" void crx_stats_desc_default(crx_stats_desc* d, int n_opp_max, int n_cars, double lap_length, double track_width) {
    memset(d, 0, sizeof(*d));
    d->n_opp_max = n_opp_max; d->n_cars = n_cars; d->degree = 6;
    d->lap_length = lap_length; d->track_width = track_width; d->l_sum = 0.4; d->w_sum = 0.2;
}

// The family's one argument check: arguments alone, before the library's state is looked at.  `which`: 0 reset, 1 one sample, 2 summary;
// a call passes the arrays it has and NULL for the rest.
static int check_stats(crx_stats_kparams& sp, int which, const crx_stats_desc* d, int batch, arr stat_i, arr stat_d, arr laps = nullptr,
                       arr xcurv = nullptr, arr car_s0 = nullptr, arr car_v = nullptr, arr car_ey = nullptr, arr n_opp = nullptr,
                       arr car_dims = nullptr, arr group = nullptr, int n_groups = 1, arr sum_i = nullptr, arr sum_d = nullptr) {
    auto positive = [](double v) { return v > 0.0 && isfinite(v); };
    if (!d) return fail(CRX_ERR_ARG, "desc is NULL");
    if (d->n_opp_max < 0 || d->n_opp_max > CRX_STATS_MAX_OPP) return fail(CRX_ERR_ARG, "n_opp_max=%d outside [0,%d]", d->n_opp_max, CRX_STATS_MAX_OPP);
    if (d->n_cars < 0 || d->n_cars > CRX_MAX_OBS + 1) return fail(CRX_ERR_ARG, "n_cars=%d outside [0,%d]", d->n_cars, CRX_MAX_OBS + 1);
    if (d->n_cars > 0 && d->n_opp_max < d->n_cars - 1) return fail(CRX_ERR_ARG, "field mode: n_opp_max=%d < n_cars - 1 = %d", d->n_opp_max, d->n_cars - 1);
    if (d->degree < 2 || d->degree > 8 || (d->degree & 1)) return fail(CRX_ERR_ARG, "degree must be 2, 4, 6 or 8");
    if (!positive(d->lap_length) || !positive(d->l_sum) || !positive(d->w_sum) || !(d->track_width > 0.0))
        return fail(CRX_ERR_ARG, "lap_length, l_sum and w_sum must be positive and finite, track_width positive");
    if (batch < 0) return fail(CRX_ERR_ARG, "batch < 0");
    if (d->n_cars > 0 && batch % d->n_cars) return fail(CRX_ERR_ARG, "field mode: batch=%d is not a multiple of n_cars=%d", batch, d->n_cars);
    if (which == 1) {
        if (d->n_cars > 0 && (car_s0 || car_v || car_ey || n_opp)) return fail(CRX_ERR_ARG, "field mode takes no scripted-car arrays (car_s0, car_v, car_ey, n_opp)");
        if (d->n_cars == 0 && car_dims) return fail(CRX_ERR_ARG, "scripted mode takes no car_dims");
        if (d->n_cars == 0 && d->n_opp_max > 0 && any_null(car_s0, car_v, car_ey))
            return fail(CRX_ERR_ARG, "scripted mode with n_opp_max=%d needs car_s0, car_v and car_ey", d->n_opp_max);
    }
    if (which == 2 && group && n_groups < 1) return fail(CRX_ERR_ARG, "group given with n_groups=%d < 1", n_groups);
    if (batch > 0 && (any_null(stat_i, stat_d) || (which < 2 && !laps) || (which == 1 && !xcurv))) return fail(CRX_ERR_ARG, "NULL array argument");
    if (which == 2 && any_null(sum_i, sum_d)) return fail(CRX_ERR_ARG, "NULL array argument");
    memset(&sp, 0, sizeof(sp));
    sp.d = *d; sp.batch = batch; sp.n_groups = group ? n_groups : 1;
    return 0;
}

extern "C" {

int crx_race_stats_reset_dev(const crx_stats_desc* d, int batch, const int32_t* laps, int32_t* stat_i, double* stat_d, void* stream) {
    crx_stats_kparams sp;
    if (int rc = check_stats(sp, 0, d, batch, stat_i, stat_d, laps)) return rc;
    if (int rc = ensure_init()) return rc;
    if (batch == 0) return CRX_OK;
    sp.laps = laps; sp.stat_i = stat_i; sp.stat_d = stat_d;
    return launched(crx_launch_race_stats(0, sp, (hipStream_t)stream), "race stats reset");
}

int crx_race_stats_dev(const crx_stats_desc* d, int batch, int sample, double t, const double* xcurv, const int32_t* laps,
                       const double* car_s0, const double* car_v, const double* car_ey, const int32_t* n_opp, const double* car_dims,
                       const double* xt, const int32_t* flag, int32_t* stat_i, double* stat_d, void* stream) {
    crx_stats_kparams sp;
    if (int rc = check_stats(sp, 1, d, batch, stat_i, stat_d, laps, xcurv, car_s0, car_v, car_ey, n_opp, car_dims)) return rc;
    if (int rc = ensure_init()) return rc;
    if (batch == 0) return CRX_OK;
    sp.sample = sample; sp.t = t; sp.xcurv = xcurv; sp.laps = laps; sp.car_s0 = car_s0; sp.car_v = car_v; sp.car_ey = car_ey; sp.n_opp = n_opp;
    sp.car_dims = car_dims; sp.xt = xt; sp.flag = flag; sp.stat_i = stat_i; sp.stat_d = stat_d;
    return launched(crx_launch_race_stats(1, sp, (hipStream_t)stream), "race stats");
}

int crx_race_stats_laps_dev(const crx_stats_desc* d, int batch, int sample, double t, const double* lap_length, const double* xcurv,
                            const int32_t* laps, const double* car_s0, const double* car_v, const double* car_ey, const int32_t* n_opp,
                            const double* car_dims, const double* xt, const int32_t* flag, int32_t* stat_i, double* stat_d, void* stream) {
    crx_stats_kparams_laps sp;
    if (int rc = check_stats(sp, 1, d, batch, stat_i, stat_d, laps, xcurv, car_s0, car_v, car_ey, n_opp, car_dims)) return rc;
    if (batch > 0 && !lap_length) return fail(CRX_ERR_ARG, "NULL array argument");
    if (int rc = ensure_init()) return rc;
    if (batch == 0) return CRX_OK;
    sp.sample = sample; sp.t = t; sp.xcurv = xcurv; sp.laps = laps; sp.car_s0 = car_s0; sp.car_v = car_v; sp.car_ey = car_ey; sp.n_opp = n_opp;
    sp.car_dims = car_dims; sp.xt = xt; sp.flag = flag; sp.stat_i = stat_i; sp.stat_d = stat_d; sp.lap_lengths = lap_length;
    return launched(crx_launch_race_stats_laps(sp, (hipStream_t)stream), "race stats (per-car lap lengths)");
}

int crx_race_stats_summary_dev(const crx_stats_desc* d, int batch, const int32_t* group, int n_groups, const int32_t* stat_i,
                               const double* stat_d, int64_t* sum_i, double* sum_d, void* stream) {
    crx_stats_kparams sp;
    if (int rc = check_stats(sp, 2, d, batch, stat_i, stat_d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, group, n_groups,
                             sum_i, sum_d)) return rc;
    if (int rc = ensure_init()) return rc;
    sp.group = group; sp.stat_i = (int32_t*)stat_i; sp.stat_d = (double*)stat_d; sp.sum_i = (long long*)sum_i; sp.sum_d = sum_d;
    return launched(crx_launch_race_stats(2, sp, (hipStream_t)stream), "race stats summary");   // (batch == 0: the records of empty groups)
}

// host-pointer twins: stat_i / stat_d travel both ways
int crx_race_stats_reset(const crx_stats_desc* d, int batch, const int32_t* laps, int32_t* stat_i, double* stat_d) {
    crx_stats_kparams chk;
    if (int rc = check_stats(chk, 0, d, batch, stat_i, stat_d, laps)) return rc;
    if (int rc = ensure_init()) return rc;
    if (batch == 0) return CRX_OK;
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    const size_t Bn = (size_t)batch;
    Stage sg;
    auto dl = sg.in(laps, Bn);
    auto dsi = sg.out(stat_i, Bn * CRX_STATS_NI); auto dsd = sg.out(stat_d, Bn * (CRX_STATS_ND + d->n_opp_max));
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_race_stats_reset_dev(d, batch, sg[dl], sg[dsi], sg[dsd], g_stream)) return rc;
    return sg.down(g_stream);
}

int crx_race_stats(const crx_stats_desc* d, int batch, int sample, double t, const double* xcurv, const int32_t* laps, const double* car_s0,
                   const double* car_v, const double* car_ey, const int32_t* n_opp, const double* car_dims, const double* xt,
                   const int32_t* flag, int32_t* stat_i, double* stat_d) {
    crx_stats_kparams chk;
    if (int rc = check_stats(chk, 1, d, batch, stat_i, stat_d, laps, xcurv, car_s0, car_v, car_ey, n_opp, car_dims)) return rc;
    if (int rc = ensure_init()) return rc;
    if (batch == 0) return CRX_OK;
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    const size_t Bn = (size_t)batch, V = (size_t)d->n_opp_max;
    Stage sg;
    auto opt_d = [&](const double* p, size_t n) { return p ? sg.in(p, n) : Stage::Ref<double>{}; };   // unused: sg[ref] is NULL
    auto opt_i = [&](const int32_t* p, size_t n) { return p ? sg.in(p, n) : Stage::Ref<int32_t>{}; };
    auto dx = sg.in(xcurv, Bn * 6); auto dl = sg.in(laps, Bn);
    auto ds0 = opt_d(car_s0, Bn * V), dv = opt_d(car_v, Bn * V), dey = opt_d(car_ey, Bn * V), dcd = opt_d(car_dims, Bn * 2), dxt = opt_d(xt, Bn * 6);
    auto dno = opt_i(n_opp, Bn), dfl = opt_i(flag, Bn);
    auto dsi = sg.inout(stat_i, Bn * CRX_STATS_NI); auto dsd = sg.inout(stat_d, Bn * (CRX_STATS_ND + V));
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_race_stats_dev(d, batch, sample, t, sg[dx], sg[dl], sg[ds0], sg[dv], sg[dey], sg[dno], sg[dcd], sg[dxt], sg[dfl], sg[dsi],
                                    sg[dsd], g_stream)) return rc;
    return sg.down(g_stream);
}

int crx_race_stats_summary(const crx_stats_desc* d, int batch, const int32_t* group, int n_groups, const int32_t* stat_i, const double* stat_d,
                           int64_t* sum_i, double* sum_d) {
    crx_stats_kparams chk;
    if (int rc = check_stats(chk, 2, d, batch, stat_i, stat_d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, group, n_groups,
                             sum_i, sum_d)) return rc;
    if (int rc = ensure_init()) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    HIP_TRY(hipSetDevice(g_device));
    const size_t Bn = (size_t)batch, G = (size_t)chk.n_groups;
    Stage sg;
    auto dg = group ? sg.in(group, Bn) : Stage::Ref<int32_t>{};
    auto dsi = sg.in(stat_i, Bn * CRX_STATS_NI); auto dsd = sg.in(stat_d, Bn * (CRX_STATS_ND + d->n_opp_max));
    auto doi = sg.out(sum_i, G * CRX_STATS_SUM_NI); auto dod = sg.out(sum_d, G * CRX_STATS_SUM_ND);
    if (int rc = sg.up(g_stream)) return rc;
    if (int rc = crx_race_stats_summary_dev(d, batch, sg[dg], chk.n_groups, sg[dsi], sg[dsd], sg[doi], sg[dod], g_stream)) return rc;
    return sg.down(g_stream);
}

}  // extern "C"

// ---- multi-GPU: the ONE collective of the planner sweep, on RCCL directly ----------------------------------------
// One process per GPU; the caller owns the rendezvous (it carries the 128-byte id from rank 0 to the others by whatever
// it has: MPI, a file, torch.distributed's store).  RCCL is resolved at run time: if the process already holds a librccl
// (PyTorch-ROCm bundles one under the SONAME librccl.so.1) that copy is used -- two RCCL instances in one process would
// each build their own topology and IPC state -- otherwise /opt/rocm's is loaded.  libcrx therefore has no link-time
// dependency on RCCL, and single-GPU users never load it.
namespace {
struct RcclApi {
    void* h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
} g_rccl;
ncclComm_t g_comm = nullptr;
int g_world = 0, g_rank = -1;

int rccl_bind() {
    if (g_rccl.AllGather) return CRX_OK;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    for (const char* n : names) if ((h = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;     // a copy the process already holds
    if (!h) for (const char* n : names) if ((h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!h) return fail(CRX_ERR_HIP, "RCCL not found (librccl.so.1): %s", dlerror());
    g_rccl.h = h;
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))dlsym(h, "ncclCommInitRank");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(h, "ncclCommDestroy");
    g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))dlsym(h, "ncclGetErrorString");
    auto ag = (decltype(g_rccl.AllGather))dlsym(h, "ncclAllGather");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.CommDestroy || !g_rccl.GetErrorString || !ag)
        return fail(CRX_ERR_HIP, "librccl lacks an expected entry point");
    g_rccl.AllGather = ag;
    return CRX_OK;
}
#define RCCL_TRY(expr)                                                                                    \
    do {                                                                                                  \
        ncclResult_t r_ = (expr);                                                                         \
        if (r_ != ncclSuccess) return fail(CRX_ERR_HIP, "%s: %s", #expr, g_rccl.GetErrorString(r_));      \
    } while (0)

// winner record = {int32 flag; int32 status; double X[N+1][6]}: 8 + 624 = 632 B at N = 12, carried as 1 + 6 (N + 1)
// 8-byte words (word 0 = the two int32, bit for bit; the collective only moves bytes); rows past n_local are zero
__global__ void __launch_bounds__(256) crx_pack_winners_kernel(int n_local, int n_max, int rec, const int32_t* flag, const int32_t* status,
                                                               const double* best_X, double* send) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n_max * rec) return;
    const size_t s = i / rec;
    const int c = (int)(i - s * rec);
    double v = 0.0;
    if (s < (size_t)n_local) {
        if (c == 0) {
            const unsigned long long w = (unsigned long long)(uint32_t)flag[s] | ((unsigned long long)(uint32_t)(status ? status[s] : 0) << 32);
            v = __longlong_as_double((long long)w);
        } else {
            v = best_X[s * (rec - 1) + (c - 1)];
        }
    }
    send[i] = v;
}
}  // namespace

extern "C" {

int crx_comm_get_unique_id(void* id) {
    if (!id) return fail(CRX_ERR_ARG, "id is NULL");
    if (int rc = ensure_init()) return rc;
    if (int rc = rccl_bind()) return rc;
    static_assert(sizeof(ncclUniqueId) == CRX_COMM_ID_BYTES, "id size");
    RCCL_TRY(g_rccl.GetUniqueId((ncclUniqueId*)id));
    return CRX_OK;
}

int crx_comm_init_rank(const void* id, int world, int rank) {
    if (!id || world < 1 || rank < 0 || rank >= world) return fail(CRX_ERR_ARG, "bad communicator arguments (world %d, rank %d)", world, rank);
    if (int rc = ensure_init()) return rc;
    if (int rc = rccl_bind()) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_comm) return fail(CRX_ERR_ARG, "communicator already initialised (crx_comm_destroy first)");
    HIP_TRY(hipSetDevice(g_device));
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    RCCL_TRY(g_rccl.CommInitRank(&g_comm, world, uid, rank));
    g_world = world; g_rank = rank;
    return CRX_OK;
}

// one wavefront that keeps a CU busy for `ticks` of the constant 100 MHz clock: two of them on two streams finish in the time of
// one if, and only if, the streams sit on different hardware queues
__global__ void __launch_bounds__(64) crx_spin_kernel(long long ticks) {
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

static double spin_ms(hipStream_t a, hipStream_t b, long long ticks) {
    const auto t0 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(crx_spin_kernel, dim3(1), dim3(64), 0, a, ticks);
    if (b) hipLaunchKernelGGL(crx_spin_kernel, dim3(1), dim3(64), 0, b, ticks);
    (void)hipStreamSynchronize(a);
    if (b) (void)hipStreamSynchronize(b);
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int crx_streams_create(int n, void** streams, int* n_concurrent) {
    if (int rc = ensure_init()) return rc;
    if (n < 0 || n > 64 || (n > 0 && !streams)) return fail(CRX_ERR_ARG, "bad stream count / NULL array");
    if (n_concurrent) *n_concurrent = 0;
    if (n == 0) return CRX_OK;
    HIP_TRY(hipSetDevice(g_device));
    // candidates: more than asked for, so that a set of n on pairwise different queues can be picked (if the runtime has that many)
    const int m = n + 8;
    std::vector<hipStream_t> cand(m, nullptr);
    for (int i = 0; i < m; i++) {
        hipError_t e = hipStreamCreateWithFlags(&cand[i], hipStreamNonBlocking);
        if (e != hipSuccess) {
            for (int j2 = 0; j2 < i; j2++) (void)hipStreamDestroy(cand[j2]);
            return fail(CRX_ERR_HIP, "hipStreamCreateWithFlags: %s", hipGetErrorString(e));
        }
    }
    const long long ticks = 15000;   // 150 us
    for (int i = 0; i < m; i++) (void)spin_ms(cand[i], nullptr, 100);   // first use: the runtime binds the queue, the kernel is loaded
    double single = 1e30;
    for (int i = 0; i < m; i++) single = fmin(single, spin_ms(cand[i], nullptr, ticks));
    // greedy: a stream joins the set if a pair of spins with every member takes the time of one (twice measured, the faster counts)
    std::vector<int> pick;
    for (int i = 0; i < m && (int)pick.size() < n; i++) {
        bool ok = true;
        for (int p : pick) {
            const double t = fmin(spin_ms(cand[p], cand[i], ticks), spin_ms(cand[p], cand[i], ticks));
            if (t > 1.6 * single) { ok = false; break; }
        }
        if (ok) pick.push_back(i);
    }
    const int nc = (int)pick.size();
    std::vector<char> used(m, 0);
    for (int p : pick) used[p] = 1;
    for (int i = 0; i < m && (int)pick.size() < n; i++)      // fewer queues than streams asked for: the rest share
        if (!used[i]) { pick.push_back(i); used[i] = 1; }
    for (int i = 0; i < n; i++) streams[i] = (void*)cand[pick[i]];
    for (int i = 0; i < m; i++)
        if (!used[i]) (void)hipStreamDestroy(cand[i]);
    if (n_concurrent) *n_concurrent = nc;
    return CRX_OK;
}

int crx_streams_destroy(int n, void** streams) {
    if (n < 0 || (n > 0 && !streams)) return fail(CRX_ERR_ARG, "bad stream count / NULL array");
    int rc = CRX_OK;
    for (int i = 0; i < n; i++) {
        if (!streams[i]) continue;
        (void)hipStreamSynchronize((hipStream_t)streams[i]);
        if (hipStreamDestroy((hipStream_t)streams[i]) != hipSuccess) rc = fail(CRX_ERR_HIP, "hipStreamDestroy failed");
        streams[i] = nullptr;
    }
    return rc;
}

int crx_comm_world(void) { return g_comm ? g_world : 0; }
int crx_comm_rank(void) { return g_comm ? g_rank : -1; }

int crx_comm_destroy(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_comm) return CRX_OK;
    RCCL_TRY(g_rccl.CommDestroy(g_comm));
    g_comm = nullptr; g_world = 0; g_rank = -1;
    return CRX_OK;
}

int crx_allgather_winners_dev(int n_local, int n_max, int N, const int32_t* flag, const int32_t* status, const double* best_X, double* send,
                              double* recv, void* stream) {
    if (int rc = ensure_init()) return rc;
    if (!g_comm) return fail(CRX_ERR_ARG, "no communicator (crx_comm_init_rank)");
    if (n_local < 0 || n_max < n_local || N < 1 || N > CRX_MAX_N) return fail(CRX_ERR_ARG, "bad sizes (n_local %d, n_max %d, N %d)", n_local, n_max, N);
    if (n_max == 0) return CRX_OK;
    if (!send || !recv || (n_local > 0 && (!flag || !best_X))) return fail(CRX_ERR_ARG, "NULL array argument");
    const int rec = 1 + (N + 1) * 6;
    const size_t cnt = (size_t)n_max * rec;
    hipLaunchKernelGGL(crx_pack_winners_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_local, n_max, rec, flag,
                       status, best_X, send);
    HIP_TRY(hipGetLastError());
    RCCL_TRY(g_rccl.AllGather(send, recv, cnt, ncclFloat64, g_comm, (hipStream_t)stream));
    return CRX_OK;
}

}  // extern "C"
