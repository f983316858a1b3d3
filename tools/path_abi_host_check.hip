// Stand-alone driver of crx_api.hip's path-planner host code (crx_path_prep / crx_path_plan: argument checks, host validation of
// n_veh / order, the self-sizing staging incl. in/out arrays and the scratch block) for a sanitizer build on the CPU, no GPU:
// the HIP runtime calls the API layer makes are answered from the heap, the three launchers of crx_pathplan.hip by host loops that
// touch every array element the kernels may touch.  Build and run from car-racing_amd/csrc after `make` (the other units' objects
// supply the launchers this driver does not replace):
//     S="-Xarch_host -fsanitize=address,undefined"
//     hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -DCRX_NFIX_LIST=10,12,20 $S -c crx_api.hip -o /tmp/crx_api_san.o
//     hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -I. $S -c ../../tools/path_abi_host_check.hip -o /tmp/path_abi_host_check.o
//     hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/path_abi_host_check.o /tmp/crx_api_san.o \
//           $(ls *.o | grep -v -e '^crx_api.o$' -e '^crx_pathplan.o$') -o /tmp/path_abi_host_check && /tmp/path_abi_host_check
// It is its own program: nothing here is loaded into Python, and it is not part of the test suite.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "crx_kparams.h"

static int g_have_device = 0;
extern "C" {
hipError_t hipGetDeviceCount(int* n) { *n = g_have_device; return g_have_device ? hipSuccess : hipErrorNoDevice; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = (hipStream_t)malloc(8); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { free(s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipMalloc(void** p, size_t n) { *p = malloc(n); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) { free(p); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { *p = malloc(n); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
}

// host stand-ins of the three kernels: every array element the real kernels may touch is read / written here
static int g_launches = 0;
hipError_t crx_launch_pathprep(const crx_pathplan_kparams& pp, hipStream_t) {
    const int N1 = pp.d.N + 1, V = pp.d.n_veh_max, R = V + 1, VA = pp.d.n_all_max;
    g_launches++;
    for (int s = 0; s < pp.n_scen; s++) {
        const int nv = pp.n_veh[s];
        const bool skip = nv == 0 || (pp.active && pp.active[s] == 0);
        for (int r = 0; r < R; r++) {
            if (pp.qp_active) pp.qp_active[s * R + r] = !skip;
            if (skip) continue;
            double acc = pp.x_wrapped[6 * s + 5] + pp.x_raw[6 * s + 5] + pp.max_dv[s] + pp.opt_s[pp.d.n_opt - 1] + pp.opt_ey[pp.d.n_opt - 1];
            for (int k = 0; k < nv; k++) acc += pp.veh_xcurv[(s * VA + pp.order[s * V + k]) * 6 + 5] + pp.obs_ey[(s * V + k) * N1 + N1 - 1];
            for (int j = 0; j < N1; j++) {
                const size_t o = ((size_t)s * R + r) * N1 + j;
                pp.opt[o] = acc; pp.bez[o] = r; pp.lb[o] = -1.0; pp.ub[o] = j;
            }
            pp.e0[s * R + r] = s; pp.eN[s * R + r] = r;
        }
        if (!skip) pp.span[s] = 100.0 + s;
    }
    return hipSuccess;
}
hipError_t crx_launch_path_masked(const crx_path_kparams_masked& pp, hipStream_t) {
    const int N1 = pp.N + 1;
    g_launches++;
    for (int b = 0; b < pp.batch; b++) {
        if (pp.active && pp.active[b] == 0) { pp.cost[b] = INFINITY; pp.status[b] = CRX_SKIPPED; pp.iters[b] = 0; continue; }
        for (int j = 0; j < N1; j++) pp.E[(size_t)b * N1 + j] = pp.opt[(size_t)b * N1 + j] + pp.bez[(size_t)b * N1 + j] + pp.ub[(size_t)b * N1 + j] + pp.lb[(size_t)b * N1 + j];
        pp.cost[b] = pp.e0[b] + pp.eN[b]; pp.status[b] = 0; pp.kkt[b] = 1e-9; pp.iters[b] = 7;
    }
    return hipSuccess;
}
hipError_t crx_launch_pathselect(const crx_pathplan_kparams& pp, hipStream_t) {
    const int N1 = pp.d.N + 1, R = pp.d.n_veh_max + 1;
    g_launches++;
    for (int s = 0; s < pp.n_scen; s++) {
        if (pp.n_veh[s] == 0 || (pp.active && pp.active[s] == 0)) { pp.flag[s] = -1; pp.plan_status[s] = CRX_SKIPPED; continue; }
        pp.flag[s] = pp.n_veh[s]; pp.plan_status[s] = 0;
        for (int e = 0; e < 6 * N1; e++) pp.target[(size_t)s * N1 * 6 + e] = pp.span[s] + pp.E[((size_t)s * R + pp.n_veh[s]) * N1 + e / 6] + pp.opt_vx[0] + pp.cost[s * R];
    }
    return hipSuccess;
}

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s  [%s]\n", __LINE__, #c, crx_last_error()); return 1; } } while (0)

struct Case {
    int S, N, V, VA, T;
    std::vector<double> xw, xr, veh, mdv, oe, ts, te, tv, E, cost, kkt, target, opt, bez, lb, ub, e0, eN, span;
    std::vector<int32_t> nv, order, active, status, iters, flag, ps;
    Case(int S_, int N_, int V_, int VA_, int T_) : S(S_), N(N_), V(V_), VA(VA_), T(T_) {
        const int N1 = N + 1, R = V + 1;
        xw.assign(S * 6, 0.5); xr.assign(S * 6, 0.25); veh.assign((size_t)S * VA * 6, 0.125); mdv.assign(S, 1.0); oe.assign((size_t)S * V * N1, 2.0);
        ts.assign(T, 3.0); te.assign(T, 4.0); tv.assign(T, 5.0);
        E.assign((size_t)S * R * N1, -7.0); cost.assign(S * R, -7.0); kkt.assign(S * R, -7.0); target.assign((size_t)S * N1 * 6, -7.0);
        opt.assign((size_t)S * R * N1, -7.0); bez = lb = ub = opt; e0.assign(S * R, -7.0); eN = e0; span.assign(S, -7.0);
        nv.assign(S, 0); order.assign(S * V, -1); active.assign(S, 1); status.assign(S * R, -7); iters.assign(S * R, -7); flag.assign(S, -7); ps.assign(S, -7);
        for (int s = 0; s < S; s++) {
            nv[s] = s % (V + 1);
            for (int k = 0; k < nv[s]; k++) order[s * V + k] = (s + k) % VA;
            if (s % 5 == 3) active[s] = 0;
        }
    }
    int plan(const crx_pathprep_desc* d, const crx_path_desc* qd, bool with_active) {
        return crx_path_plan(d, qd, S, with_active ? active.data() : nullptr, xw.data(), xr.data(), nv.data(), order.data(), veh.data(), mdv.data(), oe.data(),
                             ts.data(), te.data(), tv.data(), E.data(), cost.data(), status.data(), kkt.data(), iters.data(), flag.data(), target.data(), ps.data());
    }
    int prep(const crx_pathprep_desc* d) {
        return crx_path_prep(d, S, xw.data(), xr.data(), nv.data(), order.data(), veh.data(), mdv.data(), oe.data(), ts.data(), te.data(), opt.data(), bez.data(),
                             lb.data(), ub.data(), e0.data(), eN.data(), span.data());
    }
};

static int verify(Case& c, bool with_active) {
    const int N1 = c.N + 1, R = c.V + 1;
    for (int s = 0; s < c.S; s++) {
        const bool skip = c.nv[s] == 0 || (with_active && c.active[s] == 0);
        CHECK(c.flag[s] == (skip ? -1 : c.nv[s]) && c.ps[s] == (skip ? CRX_SKIPPED : 0));
        for (int r = 0; r < R; r++) {
            const int b = s * R + r;
            CHECK(c.status[b] == (skip ? CRX_SKIPPED : 0) && c.iters[b] == (skip ? 0 : 7));
            CHECK(skip ? (isinf(c.cost[b]) && c.kkt[b] == -7.0) : (c.cost[b] == s + r && c.kkt[b] == 1e-9));
            double acc = 0.5 + 0.25 + 1.0 + 3.0 + 4.0 + c.nv[s] * (0.125 + 2.0);
            for (int j = 0; j < N1; j++) CHECK(c.E[(size_t)b * N1 + j] == (skip ? -7.0 : acc + r - 1.0 + j));
        }
        for (int e = 0; e < 6 * N1; e++) {
            const double acc = 0.5 + 0.25 + 1.0 + 3.0 + 4.0 + c.nv[s] * (0.125 + 2.0);
            CHECK(c.target[(size_t)s * N1 * 6 + e] == (skip ? -7.0 : (100.0 + s) + (acc + c.nv[s] - 1.0 + e / 6) + 5.0 + (s + 0)));
        }
    }
    return 0;
}

int main() {
    crx_pathprep_desc d, bad;
    crx_path_desc qd, qbad;
    const int N = 10, V = 3, VA = 5, T = 40;
    crx_pathprep_desc_default(&d, N, V, VA, T, 1.0, 19.25);
    crx_path_desc_default(&qd, N, 0.98);
    Case c(7, N, V, VA, T);
    // refusals, before and after init: the same answers
    for (int pass = 0; pass < 2; pass++) {
        bad = d; bad.N = CRX_MAX_N + 1; CHECK(c.plan(&bad, &qd, true) == CRX_ERR_ARG && c.prep(&bad) == CRX_ERR_ARG);
        bad = d; bad.N = 1; CHECK(c.plan(&bad, &qd, true) == CRX_ERR_ARG);
        bad = d; bad.n_veh_max = CRX_MAX_VEH + 1; CHECK(c.plan(&bad, &qd, true) == CRX_ERR_ARG && c.prep(&bad) == CRX_ERR_ARG);
        bad = d; bad.n_veh_max = 0; CHECK(c.prep(&bad) == CRX_ERR_ARG);
        bad = d; bad.n_all_max = 0; CHECK(c.prep(&bad) == CRX_ERR_ARG);
        bad = d; bad.n_opt = 1; CHECK(c.prep(&bad) == CRX_ERR_ARG);
        bad = d; bad.lap_length = 0.0; CHECK(c.prep(&bad) == CRX_ERR_ARG);
        bad = d; bad.track_width = NAN; CHECK(c.prep(&bad) == CRX_ERR_ARG);
        qbad = qd; qbad.N = N + 1; CHECK(c.plan(&d, &qbad, true) == CRX_ERR_ARG);
        qbad = qd; qbad.alpha = 1.5; CHECK(c.plan(&d, &qbad, true) == CRX_ERR_ARG);
        CHECK(c.plan(nullptr, &qd, true) == CRX_ERR_ARG && c.plan(&d, nullptr, true) == CRX_ERR_ARG && c.prep(nullptr) == CRX_ERR_ARG);
        CHECK(crx_path_plan(&d, &qd, -1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, nullptr, nullptr, nullptr) == CRX_ERR_ARG);
        CHECK(crx_path_plan(&d, &qd, 3, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, nullptr, nullptr, nullptr) == CRX_ERR_ARG);
        CHECK(crx_path_prep(&d, 3, c.xw.data(), c.xr.data(), c.nv.data(), c.order.data(), c.veh.data(), c.mdv.data(), c.oe.data(), c.ts.data(), c.te.data(), c.opt.data(),
                            c.bez.data(), c.lb.data(), c.ub.data(), c.e0.data(), c.eN.data(), nullptr) == CRX_ERR_ARG);
        if (pass == 0) {
            CHECK(c.plan(&d, &qd, true) == CRX_ERR_NOT_INIT && c.prep(&d) == CRX_ERR_NOT_INIT);
            CHECK(crx_init(0) == CRX_ERR_NO_DEVICE);
            g_have_device = 1;
            CHECK(crx_init(0) == CRX_OK);
        }
    }
    CHECK(g_launches == 0);
    // host-side validation of n_veh / order
    { Case e(4, N, V, VA, T); e.nv[2] = V + 1; CHECK(e.plan(&d, &qd, true) == CRX_ERR_ARG && e.prep(&d) == CRX_ERR_ARG); }
    { Case e(4, N, V, VA, T); e.order[3 * V] = VA; CHECK(e.plan(&d, &qd, true) == CRX_ERR_ARG && e.prep(&d) == CRX_ERR_ARG); }
    CHECK(g_launches == 0);
    // empty batch
    { Case e(0, N, V, VA, T); CHECK(e.plan(&d, &qd, true) == CRX_OK && e.prep(&d) == CRX_OK); }
    CHECK(g_launches == 0);
    // staged calls: small, then larger (the staging grows), then small again; with and without a mask; other horizons and vehicle counts
    const int sizes[] = {7, 300, 1, 64};
    for (int S : sizes)
        for (int with_active = 0; with_active < 2; with_active++) {
            Case e(S, N, V, VA, T);
            CHECK(e.plan(&d, &qd, with_active != 0) == CRX_OK);
            if (verify(e, with_active != 0)) return 1;
            Case f(S, N, V, VA, T);
            CHECK(f.prep(&d) == CRX_OK);
            for (int s = 0; s < S; s++) CHECK(f.span[s] == (f.nv[s] ? 100.0 + s : -7.0) && f.ub[((size_t)s * (V + 1) + V) * (N + 1) + N] == (f.nv[s] ? N : -7.0));
        }
    crx_pathprep_desc d2;
    crx_path_desc q2;
    crx_pathprep_desc_default(&d2, CRX_MAX_N, CRX_MAX_VEH, 9, 3, 2.5, 19.25);
    crx_path_desc_default(&q2, CRX_MAX_N, 0.5);
    { Case e(33, CRX_MAX_N, CRX_MAX_VEH, 9, 3); CHECK(e.plan(&d2, &q2, true) == CRX_OK); if (verify(e, true)) return 1; }
    crx_pathprep_desc_default(&d2, 2, 1, 1, 2, 2.5, 19.25);
    crx_path_desc_default(&q2, 2, 0.5);
    { Case e(5, 2, 1, 1, 2); CHECK(e.plan(&d2, &q2, false) == CRX_OK); if (verify(e, false)) return 1; }
    crx_shutdown();
    printf("path-planner ABI host code: all checks passed (%d stand-in launches)\n", g_launches);
    return 0;
}
