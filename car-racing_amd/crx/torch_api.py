"""Device-resident entry points: torch CUDA(HIP) tensors in, torch tensors out, no host staging.

torch is used for device memory, streams and torch.distributed only; the solve itself is
libcrx's `*_dev` C ABI called with raw device pointers on torch's current stream.
"""
import ctypes as C

import torch

from . import _state, abi, binding, lib


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _chk(t, dtype, shape, name):
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError("%s: expected contiguous cuda %s tensor of shape %s, got %s %s %s" % (
            name, dtype, tuple(shape), t.device, t.dtype, tuple(t.shape)))
    # the *_dev entry points launch on the device libcrx was initialised on: a tensor living elsewhere would be
    # dereferenced on the wrong GPU
    dev = _state["device"]
    if dev is not None and t.device.index != dev:
        raise ValueError("%s lives on %s but libcrx was initialised on cuda:%d (crx.init(device))" % (name, t.device, dev))
    return t


def _call(name, *args):
    binding()
    L = lib()
    fn = getattr(L, name)
    fn.restype = C.c_int
    rc = fn(*args)
    if rc != 0:
        raise RuntimeError("%s failed: rc=%d %s" % (name, rc, (L.crx_last_error() or b"").decode()))


def _stream():
    binding()
    return C.c_void_p(torch.cuda.current_stream(torch.device("cuda", _state["device"])).cuda_stream)


def new_streams(n, device=None):
    """crx_streams_create: n HIP streams of which the first `n_concurrent` were MEASURED to sit on pairwise different hardware
    queues (torch's own stream pool gives no such guarantee: include/crx.h "Streams"), wrapped as torch.cuda.ExternalStream.
    Returns (streams, n_concurrent).  They live as long as the process."""
    binding()
    arr = (C.c_void_p * n)()
    nc = C.c_int(0)
    _call("crx_streams_create", C.c_int(n), arr, C.byref(nc))
    dev = torch.device("cuda", _state["device"]) if device is None else torch.device(device)
    return [torch.cuda.ExternalStream(int(arr[i]), device=dev) for i in range(n)], int(nc.value)


class Timer:
    """crx_timer_* (include/crx.h): device time of what is enqueued between begin() and end() on torch's current stream."""

    def __init__(self):
        binding()
        self.h = C.c_void_p(0)
        _call("crx_timer_create", C.byref(self.h))

    def begin(self):
        _call("crx_timer_begin", self.h, _stream())

    def end(self):
        _call("crx_timer_end", self.h, _stream())

    def ms(self):
        return float(lib().crx_timer_ms(self.h))

    def __del__(self):
        try:
            if self.h:
                lib().crx_timer_destroy(self.h)
        except Exception:
            pass


class CbfWorkspace:
    """Pre-allocated outputs for repeated cbf_solve_dev calls of one shape."""

    def __init__(self, desc, batch, device):
        N, V = desc.N, max(desc.n_obs_max, 1)
        f64 = dict(dtype=torch.float64, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        self.X = torch.empty((batch, N + 1, 6), **f64)
        self.U = torch.empty((batch, N, 2), **f64)
        self.sigma = torch.empty((batch, V, N + 1), **f64)
        self.cost = torch.empty(batch, **f64)
        self.kkt = torch.empty(batch, **f64)
        self.status = torch.empty(batch, **i32)
        self.iters = torch.zeros(batch, **i32)


def longest_first(iters, active=None, out=None):
    """crx_order_longest_first_dev: dispatch order for the next launch from the iteration counts of the previous one (int32 [batch]
    on the device): the problems that took longest start first, masked-out ones (active == 0) last (include/crx.h, "Dispatch
    order").  Stable: equal counts keep index order."""
    Bn = iters.shape[0]
    _chk(iters, torch.int32, (Bn,), "iters")
    if active is not None:
        _chk(active, torch.int32, (Bn,), "active")
    order = out if out is not None else torch.empty(Bn, dtype=torch.int32, device=iters.device)
    _chk(order, torch.int32, (Bn,), "order")
    _call("crx_order_longest_first_dev", C.c_int(Bn), _ptr(iters), _ptr(active), _ptr(order), _stream())
    return order


def cbf_order_dev(desc, x0, xt, obs_s, obs_ey, lap_off, n_obs, obs_dims=None, active=None, out=None):
    """crx_cbf_order_dev: dispatch order of a CBF-NLP launch with no previous solve to go by, from the arguments of cbf_solve_dev --
    cars that start inside a safety ellipse first, then those whose un-steered path enters one, then the rest."""
    N, V, Bn = desc.N, desc.n_obs_max, x0.shape[0]
    _chk(x0, torch.float64, (Bn, 6), "x0")
    _chk(xt, torch.float64, (Bn, N + 1, 6) if desc.per_stage_target else (Bn, 6), "xt")
    _chk(obs_s, torch.float64, (Bn, V, N + 1), "obs_s")
    _chk(obs_ey, torch.float64, (Bn, V, N + 1), "obs_ey")
    _chk(lap_off, torch.float64, (Bn, V), "lap_off")
    _chk(n_obs, torch.int32, (Bn,), "n_obs")
    if obs_dims is not None:
        _chk(obs_dims, torch.float64, (Bn, V, 2), "obs_dims")
    if active is not None:
        _chk(active, torch.int32, (Bn,), "active")
    order = out if out is not None else torch.empty(Bn, dtype=torch.int32, device=x0.device)
    _chk(order, torch.int32, (Bn,), "order")
    _call("crx_cbf_order_dev", C.byref(desc), C.c_int(Bn), _ptr(active), _ptr(x0), _ptr(xt), _ptr(obs_s), _ptr(obs_ey), _ptr(lap_off), _ptr(n_obs),
          _ptr(obs_dims), _ptr(order), _stream())
    return order


CBF_REACH_ROW = 25   # CRX_MAX_N + 1: stride of a row of the reach table (include/crx.h CRX_CBF_MODEL_REACH_DOUBLES)


class CbfModels:
    """One LTI model per problem for cbf_solve_dev(models=...): contiguous device A [B,6,6], B [B,6,2] (e.g. what PidLaps.identify()
    returns: held, not copied) and the reach table crx_cbf_models_reach_dev computes from them -- here, once: it is valid for every solve
    with desc's N, delta_max, a_max."""

    def __init__(self, desc, A, B):
        if not (torch.is_tensor(A) and torch.is_tensor(B)) or A.dim() != 3:
            raise ValueError("CbfModels: A [B,6,6], B [B,6,2] device tensors expected")
        Bn = A.shape[0]
        self.A = _chk(A, torch.float64, (Bn, 6, 6), "models A")
        self.B = _chk(B, torch.float64, (Bn, 6, 2), "models B")
        self.batch, self.N, self.delta_max, self.a_max = Bn, desc.N, desc.delta_max, desc.a_max
        self.reach = torch.empty((Bn, 2, CBF_REACH_ROW), dtype=torch.float64, device=A.device)
        _call("crx_cbf_models_reach_dev", C.byref(desc), C.c_int(Bn), _ptr(self.A), _ptr(self.B), _ptr(self.reach), _stream())


def cbf_solve_dev(desc, x0, xt, obs_s, obs_ey, lap_off, n_obs, ws=None, active=None, obs_dims=None, order=None, models=None):
    """crx_cbf_solve_ordered_dev, the superset entry point: `active` (int32 [batch], 0 = leave the problem alone), `obs_dims`
    ([batch, n_obs_max, 2]: l_agent + l_obs, w_agent + w_obs per obstacle slot), `order` (int32 [batch] permutation: workgroup i
    solves problem order[i]; see longest_first) -- each optional.  models (a CbfModels of this batch, built for a descriptor with the
    same N, delta_max, a_max): crx_cbf_solve_models_dev, problem b on its own model (desc.A, desc.B are ignored)."""
    N, V, B = desc.N, desc.n_obs_max, x0.shape[0]
    _chk(x0, torch.float64, (B, 6), "x0")
    _chk(xt, torch.float64, (B, N + 1, 6) if desc.per_stage_target else (B, 6), "xt")
    _chk(obs_s, torch.float64, (B, V, N + 1), "obs_s")
    _chk(obs_ey, torch.float64, (B, V, N + 1), "obs_ey")
    _chk(lap_off, torch.float64, (B, V), "lap_off")
    _chk(n_obs, torch.int32, (B,), "n_obs")
    ws = ws or CbfWorkspace(desc, B, x0.device)
    if active is not None:
        _chk(active, torch.int32, (B,), "active")
    if obs_dims is not None:
        _chk(obs_dims, torch.float64, (B, V, 2), "obs_dims")
    if order is not None:
        _chk(order, torch.int32, (B,), "order")
    if models is not None:
        if not isinstance(models, CbfModels):
            raise ValueError("models: a CbfModels is expected (CbfModels(desc, A, B))")
        if models.batch != B or (models.N, models.delta_max, models.a_max) != (desc.N, desc.delta_max, desc.a_max):
            raise ValueError("models: built for batch %d, N %d, input box (%g, %g); this solve has batch %d, N %d, (%g, %g)" % (
                models.batch, models.N, models.delta_max, models.a_max, B, desc.N, desc.delta_max, desc.a_max))
        _call("crx_cbf_solve_models_dev", C.byref(desc), C.c_int(B), _ptr(active) if active is not None else None,
              _ptr(order) if order is not None else None, _ptr(x0), _ptr(models.A), _ptr(models.B), _ptr(models.reach), _ptr(xt),
              _ptr(obs_s), _ptr(obs_ey), _ptr(lap_off), _ptr(n_obs), _ptr(obs_dims), _ptr(ws.X), _ptr(ws.U), _ptr(ws.sigma), _ptr(ws.cost),
              _ptr(ws.status), _ptr(ws.kkt), _ptr(ws.iters), _stream())
        return ws
    _call("crx_cbf_solve_ordered_dev", C.byref(desc), C.c_int(B), _ptr(active) if active is not None else None,
          _ptr(order) if order is not None else None, _ptr(x0), _ptr(xt),
          _ptr(obs_s), _ptr(obs_ey), _ptr(lap_off), _ptr(n_obs), _ptr(obs_dims), _ptr(ws.X), _ptr(ws.U), _ptr(ws.sigma), _ptr(ws.cost),
          _ptr(ws.status), _ptr(ws.kkt), _ptr(ws.iters), _stream())
    return ws


class IlqrWorkspace:
    """Pre-allocated outputs for repeated ilqr_solve_dev calls of one shape."""

    def __init__(self, desc, batch, device):
        N = desc.N
        f64 = dict(dtype=torch.float64, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        self.X = torch.zeros((batch, N + 1, 6), **f64)
        self.U = torch.zeros((batch, N, 2), **f64)
        self.cost = torch.zeros(batch, **f64)
        self.status = torch.zeros(batch, **i32)
        self.iters = torch.zeros(batch, **i32)


def ilqr_solve_dev(desc, x0, xt, obs_s, obs_ey, lap_off, n_obs, ws=None, active=None, models=None):
    """crx_ilqr_solve_dev: x0, xt [B,6]; obs_s, obs_ey [B,n_obs_max,N+1]; lap_off [B,n_obs_max]; n_obs int32 [B]; `active`
    (int32 [B], 0 = leave the problem alone: status CRX_SKIPPED, outputs untouched) optional.  models = (A [B,6,6], B [B,6,2]):
    crx_ilqr_solve_models_dev, problem b on its own model (desc.A, desc.B are ignored)."""
    N, V, B = desc.N, desc.n_obs_max, x0.shape[0]
    _chk(x0, torch.float64, (B, 6), "x0")
    _chk(xt, torch.float64, (B, 6), "xt")
    _chk(obs_s, torch.float64, (B, V, N + 1), "obs_s")
    _chk(obs_ey, torch.float64, (B, V, N + 1), "obs_ey")
    _chk(lap_off, torch.float64, (B, V), "lap_off")
    _chk(n_obs, torch.int32, (B,), "n_obs")
    if active is not None:
        _chk(active, torch.int32, (B,), "active")
    ws = ws or IlqrWorkspace(desc, B, x0.device)
    if models is not None:
        mA, mB = models
        _chk(mA, torch.float64, (B, 6, 6), "models[0]")
        _chk(mB, torch.float64, (B, 6, 2), "models[1]")
        _call("crx_ilqr_solve_models_dev", C.byref(desc), C.c_int(B), _ptr(active) if active is not None else None, _ptr(x0),
              _ptr(mA), _ptr(mB), _ptr(xt), _ptr(obs_s), _ptr(obs_ey), _ptr(lap_off), _ptr(n_obs), _ptr(ws.X), _ptr(ws.U),
              _ptr(ws.cost), _ptr(ws.status), _ptr(ws.iters), _stream())
        return ws
    _call("crx_ilqr_solve_dev", C.byref(desc), C.c_int(B), _ptr(active) if active is not None else None, _ptr(x0), _ptr(xt),
          _ptr(obs_s), _ptr(obs_ey), _ptr(lap_off), _ptr(n_obs), _ptr(ws.X), _ptr(ws.U), _ptr(ws.cost), _ptr(ws.status),
          _ptr(ws.iters), _stream())
    return ws


class LqrWorkspace:
    """Pre-allocated outputs for repeated lqr_design_dev calls of one batch; P None = the kernel skips it."""

    def __init__(self, batch, device, want_P=True):
        f64 = dict(dtype=torch.float64, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        self.K = torch.zeros((batch, 2, 6), **f64)
        self.P = torch.zeros((batch, 6, 6), **f64) if want_P else None
        self.iters = torch.zeros(batch, **i32)
        self.status = torch.zeros(batch, **i32)


def lqr_design_dev(desc, A, B, ws=None, active=None):
    """crx_lqr_design_dev: A [B,6,6], B [B,6,2] device tensors (as SysidWorkspace holds them); `active` (int32 [B], 0 = leave the
    model alone: status CRX_SKIPPED, outputs untouched) optional.  Returns the workspace: K [B,2,6], P [B,6,6], iters, status."""
    Bn = A.shape[0]
    _chk(A, torch.float64, (Bn, 6, 6), "A")
    _chk(B, torch.float64, (Bn, 6, 2), "B")
    if active is not None:
        _chk(active, torch.int32, (Bn,), "active")
    ws = ws or LqrWorkspace(Bn, A.device)
    _chk(ws.K, torch.float64, (Bn, 2, 6), "ws.K")
    if ws.P is not None:
        _chk(ws.P, torch.float64, (Bn, 6, 6), "ws.P")
    _call("crx_lqr_design_dev", C.byref(desc), C.c_int(Bn), _ptr(active) if active is not None else None, _ptr(A), _ptr(B), _ptr(ws.K),
          _ptr(ws.P), _ptr(ws.iters), _ptr(ws.status), _stream())
    return ws


def lqr_step_dev(K, xcurv, xt, u):
    """crx_lqr_step_dev: u [B,2] = -K [B,2,6] (xcurv - xt), xcurv, xt [B,6]."""
    Bn = xcurv.shape[0]
    _chk(K, torch.float64, (Bn, 2, 6), "K")
    _chk(xcurv, torch.float64, (Bn, 6), "xcurv")
    _chk(xt, torch.float64, (Bn, 6), "xt")
    _chk(u, torch.float64, (Bn, 2), "u")
    _call("crx_lqr_step_dev", C.c_int(Bn), _ptr(K), _ptr(xcurv), _ptr(xt), _ptr(u), _stream())
    return u


class SysidWorkspace:
    """Outputs and device scratch of sysid_fit_dev calls for n_logs logs of at most max_log_rows rows in n_groups groups."""

    def __init__(self, desc, n_logs, n_groups, max_log_rows, device):
        f64 = dict(dtype=torch.float64, device=device)
        self.n_logs, self.n_groups, self.max_log_rows = int(n_logs), int(n_groups), int(max_log_rows)
        self.A = torch.zeros((n_groups, 6, 6), **f64)
        self.B = torch.zeros((n_groups, 6, 2), **f64)
        self.err = torch.zeros((n_groups, 2, 6), **f64)
        self.n_pairs = torch.zeros(n_groups, dtype=torch.int64, device=device)
        self.status = torch.zeros(n_groups, dtype=torch.int32, device=device)
        fn = lib().crx_sysid_workspace_bytes
        fn.restype = C.c_size_t
        self.ws_bytes = int(fn(C.byref(desc), C.c_int(n_logs), C.c_int(n_groups), C.c_int64(max_log_rows)))
        self.scratch = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)


def sysid_fit_dev(desc, x, u, offsets, group_offsets=None, max_log_rows=None, ws=None):
    """crx_sysid_fit_dev: x [rows,6], u [rows,2] float64; offsets int64 [n_logs+1]; group_offsets int32 [n_groups+1] or None (one
    fit per log).  max_log_rows bounds every log (None: read from offsets, one device-to-host copy)."""
    rows, n_logs = x.shape[0], offsets.shape[0] - 1
    _chk(x, torch.float64, (rows, 6), "x")
    _chk(u, torch.float64, (rows, 2), "u")
    _chk(offsets, torch.int64, (n_logs + 1,), "offsets")
    G = n_logs
    if group_offsets is not None:
        G = group_offsets.shape[0] - 1
        _chk(group_offsets, torch.int32, (G + 1,), "group_offsets")
    if max_log_rows is None:
        max_log_rows = int((offsets[1:] - offsets[:-1]).max().item()) if n_logs > 0 else 0
    if ws is None or ws.n_logs != n_logs or ws.n_groups != G or ws.max_log_rows < max_log_rows:
        ws = SysidWorkspace(desc, n_logs, G, max_log_rows, x.device)
    _call("crx_sysid_fit_dev", C.byref(desc), C.c_int(n_logs), _ptr(offsets), _ptr(group_offsets), C.c_int(G), C.c_int64(ws.max_log_rows),
          _ptr(x), _ptr(u), _ptr(ws.scratch), C.c_size_t(ws.ws_bytes), _ptr(ws.A), _ptr(ws.B), _ptr(ws.err), _ptr(ws.n_pairs),
          _ptr(ws.status), _stream())
    return ws


def pid_log_dev(T, row, vt, eyt, xcurv, u_prev, u_next, x_log, u_log):
    """crx_pid_log_dev: log row `row` (< 0: none) of x_log [B,T,6] / u_log [B,T,2] from (xcurv [B,6], u_prev [B,2]), then
    u_next [B,2] = control.pid(xcurv) with targets vt, eyt [B] (u_next may be None)."""
    B = xcurv.shape[0]
    _chk(xcurv, torch.float64, (B, 6), "xcurv")
    _chk(vt, torch.float64, (B,), "vt")
    _chk(eyt, torch.float64, (B,), "eyt")
    _chk(x_log, torch.float64, (B, T, 6), "x_log")
    _chk(u_log, torch.float64, (B, T, 2), "u_log")
    if u_next is not None:
        _chk(u_next, torch.float64, (B, 2), "u_next")
    if row >= 0:
        _chk(u_prev, torch.float64, (B, 2), "u_prev")
    _call("crx_pid_log_dev", C.c_int(B), C.c_int(T), C.c_int(row), _ptr(vt), _ptr(eyt), _ptr(xcurv), _ptr(u_prev if row >= 0 else None),
          _ptr(u_next), _ptr(x_log), _ptr(u_log), _stream())


class PlannerWorkspace:
    def __init__(self, desc, batch, device):
        N = desc.N
        f64 = dict(dtype=torch.float64, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        self.X = torch.empty((batch, N + 1, 6), **f64)
        self.U = torch.empty((batch, N, 2), **f64)
        self.cost = torch.empty(batch, **f64)
        self.kkt = torch.empty(batch, **f64)
        self.status = torch.empty(batch, **i32)
        self.iters = torch.empty(batch, **i32)


PLANNER_REACH_ROWS = 24   # CRX_MAX_N: stages of a problem's reach table (include/crx.h CRX_PLANNER_MODEL_REACH_DOUBLES)


class PlannerModels:
    """One LTI model per region QP for planner_solve_dev(models=...) / planner_plan_dev(models=...): contiguous device A [n,6,6], B [n,6,2]
    (e.g. what PidLaps.identify() returns) and the reach table crx_planner_models_reach_dev computes from them -- here, once: it is valid for
    every solve with desc's N, delta_max, a_max.  regions = V + 1 of a planner step: the n models are one per SCENARIO and every one is
    repeated for its regions (the C ABI indexes the models like x0, one per region QP); regions = 1 holds A, B as they are, without a copy."""

    def __init__(self, desc, A, B, regions=1):
        if not (torch.is_tensor(A) and torch.is_tensor(B)) or A.dim() != 3:
            raise ValueError("PlannerModels: A [n,6,6], B [n,6,2] device tensors expected")
        n = A.shape[0]
        _chk(A, torch.float64, (n, 6, 6), "models A")
        _chk(B, torch.float64, (n, 6, 2), "models B")
        if int(regions) < 1:
            raise ValueError("PlannerModels: regions >= 1 expected, got %r" % (regions,))
        self.regions = int(regions)
        self.A = A.repeat_interleave(self.regions, dim=0).contiguous() if self.regions > 1 else A
        self.B = B.repeat_interleave(self.regions, dim=0).contiguous() if self.regions > 1 else B
        Bn = n * self.regions
        self.batch, self.N, self.delta_max, self.a_max = Bn, desc.N, desc.delta_max, desc.a_max
        self.reach = torch.empty((Bn, PLANNER_REACH_ROWS, 7), dtype=torch.float64, device=A.device)
        _call("crx_planner_models_reach_dev", C.byref(desc), C.c_int(Bn), _ptr(self.A), _ptr(self.B), _ptr(self.reach), _stream())


def _planner_models(models, desc, B):
    if not isinstance(models, PlannerModels):
        raise ValueError("models: a PlannerModels is expected (PlannerModels(desc, A, B, regions))")
    if models.batch != B or (models.N, models.delta_max, models.a_max) != (desc.N, desc.delta_max, desc.a_max):
        raise ValueError("models: built for batch %d, N %d, input box (%g, %g); this solve has batch %d, N %d, (%g, %g)" % (
            models.batch, models.N, models.delta_max, models.a_max, B, desc.N, desc.delta_max, desc.a_max))
    return models


def planner_solve_dev(desc, x0, bez_s, bez_ey, ey_lb, ey_ub, ws=None, models=None, active=None):
    """crx_planner_solve_dev.  models (a PlannerModels of this batch, built for a descriptor with the same N, delta_max, a_max) and / or
    `active` (int32 [batch], 0 = leave the QP alone): crx_planner_solve_models_dev, QP b on its own model (desc.A, desc.B are ignored)."""
    N, B = desc.N, x0.shape[0]
    _chk(x0, torch.float64, (B, 6), "x0")
    _chk(bez_s, torch.float64, (B, N + 1), "bez_s")
    _chk(bez_ey, torch.float64, (B, N + 1), "bez_ey")
    _chk(ey_lb, torch.float64, (B, N), "ey_lb")
    _chk(ey_ub, torch.float64, (B,), "ey_ub")
    ws = ws or PlannerWorkspace(desc, B, x0.device)
    if models is not None or active is not None:
        m = _planner_models(models, desc, B) if models is not None else None
        if active is not None:
            _chk(active, torch.int32, (B,), "active")
        _call("crx_planner_solve_models_dev", C.byref(desc), C.c_int(B), _ptr(active) if active is not None else None, _ptr(x0),
              _ptr(m.A) if m else None, _ptr(m.B) if m else None, _ptr(m.reach) if m else None, _ptr(bez_s), _ptr(bez_ey), _ptr(ey_lb),
              _ptr(ey_ub), _ptr(ws.X), _ptr(ws.U), _ptr(ws.cost), _ptr(ws.status), _ptr(ws.kkt), _ptr(ws.iters), _stream())
        return ws
    _call("crx_planner_solve_dev", C.byref(desc), C.c_int(B), _ptr(x0), _ptr(bez_s), _ptr(bez_ey), _ptr(ey_lb),
          _ptr(ey_ub), _ptr(ws.X), _ptr(ws.U), _ptr(ws.cost), _ptr(ws.status), _ptr(ws.kkt), _ptr(ws.iters),
          _stream())
    return ws


class SelectWorkspace:
    def __init__(self, desc, n_scen, device):
        N, R = desc.N, desc.n_veh_max + 1
        self.flag = torch.empty(n_scen, dtype=torch.int32, device=device)
        self.sel_cost = torch.empty((n_scen, R), dtype=torch.float64, device=device)
        self.best_X = torch.empty((n_scen, N + 1, 6), dtype=torch.float64, device=device)


def select_dev(desc, n_veh, X, obs_s, obs_ey, old_flag, ws=None):
    N, V, S = desc.N, desc.n_veh_max, n_veh.shape[0]
    _chk(n_veh, torch.int32, (S,), "n_veh")
    _chk(X, torch.float64, (S, V + 1, N + 1, 6), "X")
    _chk(obs_s, torch.float64, (S, V, N + 1), "obs_s")
    _chk(obs_ey, torch.float64, (S, V, N + 1), "obs_ey")
    _chk(old_flag, torch.int32, (S,), "old_flag")
    ws = ws or SelectWorkspace(desc, S, X.device)
    _call("crx_select_dev", C.byref(desc), C.c_int(S), _ptr(n_veh), _ptr(X), _ptr(obs_s), _ptr(obs_ey),
          _ptr(old_flag), _ptr(ws.flag), _ptr(ws.sel_cost), _ptr(ws.best_X), _stream())
    return ws


class LmpcWorkspace:
    def __init__(self, desc, batch, device):
        N, M = desc.N, desc.n_ss_max
        f64 = dict(dtype=torch.float64, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        self.X = torch.empty((batch, N + 1, 6), **f64)
        self.U = torch.empty((batch, N, 2), **f64)
        self.lam = torch.empty((batch, M), **f64)
        self.cost = torch.empty(batch, **f64)
        self.kkt = torch.empty(batch, **f64)
        self.status = torch.empty(batch, **i32)
        self.iters = torch.zeros(batch, **i32)


def lmpc_solve_dev(desc, x0, u_old, A, B, Cm, ss, qfun, n_ss, ws=None, active=None, order=None):
    """crx_lmpc_solve_ordered_dev (`active`, int32 [batch], 0 = leave alone; `order`, int32 [batch] dispatch permutation; both optional).  n_ss must satisfy 1 <= n_ss <= desc.n_ss_max (checked here on the host copy the
    caller keeps; the kernel indexes LDS with it)."""
    N, M, Bn = desc.N, desc.n_ss_max, x0.shape[0]
    _chk(x0, torch.float64, (Bn, 6), "x0")
    _chk(u_old, torch.float64, (Bn, 2), "u_old")
    _chk(A, torch.float64, (Bn, N, 36), "A")
    _chk(B, torch.float64, (Bn, N, 12), "B")
    _chk(Cm, torch.float64, (Bn, N, 6), "C")
    _chk(ss, torch.float64, (Bn, 6, M), "ss")
    _chk(qfun, torch.float64, (Bn, M), "qfun")
    _chk(n_ss, torch.int32, (Bn,), "n_ss")
    ws = ws or LmpcWorkspace(desc, Bn, x0.device)
    if active is not None:
        _chk(active, torch.int32, (Bn,), "active")
    if order is not None:
        _chk(order, torch.int32, (Bn,), "order")
    _call("crx_lmpc_solve_ordered_dev", C.byref(desc), C.c_int(Bn), _ptr(active) if active is not None else None,
          _ptr(order) if order is not None else None, _ptr(x0), _ptr(u_old),
          _ptr(A), _ptr(B), _ptr(Cm), _ptr(ss), _ptr(qfun), _ptr(n_ss), _ptr(ws.X), _ptr(ws.U), _ptr(ws.lam), _ptr(ws.cost),
          _ptr(ws.status), _ptr(ws.kkt), _ptr(ws.iters), _stream())
    return ws


class PrepWorkspace:
    """Outputs of planner_prep_dev = inputs of planner_solve_dev (same layout)."""

    def __init__(self, desc, n_scen, device):
        N, R = desc.N, desc.n_veh_max + 1
        f64 = dict(dtype=torch.float64, device=device)
        self.x0 = torch.empty((n_scen * R, 6), **f64)
        self.bez_s = torch.empty((n_scen * R, N + 1), **f64)
        self.bez_ey = torch.empty((n_scen * R, N + 1), **f64)
        self.ey_lb = torch.empty((n_scen * R, N), **f64)
        self.ey_ub = torch.empty((n_scen * R,), **f64)


def planner_prep_dev(desc, x_wrapped, x_raw, n_veh, veh_info, max_dv, obs_s, obs_ey, opt_s, opt_ey, ws=None):
    N, V, T, S = desc.N, desc.n_veh_max, desc.n_opt, x_wrapped.shape[0]
    _chk(x_wrapped, torch.float64, (S, 6), "x_wrapped")
    _chk(x_raw, torch.float64, (S, 6), "x_raw")
    _chk(n_veh, torch.int32, (S,), "n_veh")
    _chk(veh_info, torch.float64, (S, V, 3), "veh_info")
    _chk(max_dv, torch.float64, (S,), "max_dv")
    _chk(obs_s, torch.float64, (S, V, N + 1), "obs_s")
    _chk(obs_ey, torch.float64, (S, V, N + 1), "obs_ey")
    _chk(opt_s, torch.float64, (T,), "opt_s")
    _chk(opt_ey, torch.float64, (T,), "opt_ey")
    ws = ws or PrepWorkspace(desc, S, x_wrapped.device)
    _call("crx_planner_prep_dev", C.byref(desc), C.c_int(S), _ptr(x_wrapped), _ptr(x_raw), _ptr(n_veh), _ptr(veh_info),
          _ptr(max_dv), _ptr(obs_s), _ptr(obs_ey), _ptr(opt_s), _ptr(opt_ey), _ptr(ws.x0), _ptr(ws.bez_s),
          _ptr(ws.bez_ey), _ptr(ws.ey_lb), _ptr(ws.ey_ub), _stream())
    return ws


def plant_step_dev(desc, track, xglob, xcurv, u, xglob_next=None, xcurv_next=None, params=None):
    """crx_plant_step_dev; returns (xglob_next, xcurv_next) (allocated unless given).  params [B,10]: one BicycleDynamicsParam set per
    vehicle (abi.plant_params; crx_plant_step_params_plain_dev), None = desc's ten values for every vehicle."""
    Bn = xglob.shape[0]
    _chk(track, torch.float64, (desc.n_seg, 6), "track")
    _chk(xglob, torch.float64, (Bn, 6), "xglob")
    _chk(xcurv, torch.float64, (Bn, 6), "xcurv")
    _chk(u, torch.float64, (Bn, 2), "u")
    xglob_next = torch.empty_like(xglob) if xglob_next is None else xglob_next
    xcurv_next = torch.empty_like(xcurv) if xcurv_next is None else xcurv_next
    if params is not None:
        _chk(params, torch.float64, (Bn, 10), "params")
        _call("crx_plant_step_params_plain_dev", C.byref(desc), C.c_int(Bn), _ptr(track), _ptr(xglob), _ptr(xcurv), _ptr(u), _ptr(params),
              _ptr(xglob_next), _ptr(xcurv_next), _stream())
        return xglob_next, xcurv_next
    _call("crx_plant_step_dev", C.byref(desc), C.c_int(Bn), _ptr(track), _ptr(xglob), _ptr(xcurv), _ptr(u),
          _ptr(xglob_next), _ptr(xcurv_next), _stream())
    return xglob_next, xcurv_next


def cbf_prep_dev(N, lap_length, t, dt, xcurv, car_s0, car_v, car_ey, obs_s, obs_ey, lap_off, n_obs, safety_time=2.0):
    """crx_cbf_prep_dev: obstacle inputs of cbf_solve_dev for scripted cars, written into the given tensors."""
    Bn, V = car_s0.shape
    _chk(xcurv, torch.float64, (Bn, 6), "xcurv")
    for name, a in (("car_s0", car_s0), ("car_v", car_v), ("car_ey", car_ey), ("lap_off", lap_off)):
        _chk(a, torch.float64, (Bn, V), name)
    _chk(obs_s, torch.float64, (Bn, V, N + 1), "obs_s")
    _chk(obs_ey, torch.float64, (Bn, V, N + 1), "obs_ey")
    _chk(n_obs, torch.int32, (Bn,), "n_obs")
    _call("crx_cbf_prep_dev", C.c_int(N), C.c_int(V), C.c_double(lap_length), C.c_double(t), C.c_double(dt),
          C.c_double(safety_time), C.c_int(Bn), _ptr(xcurv), _ptr(car_s0), _ptr(car_v), _ptr(car_ey), _ptr(obs_s),
          _ptr(obs_ey), _ptr(lap_off), _ptr(n_obs), _stream())


class FieldWorkspace:
    """Outputs of field_prep_dev for n_races races of desc.n_cars cars: the predictions pred_s, pred_ey [R,C,N+1] and the obstacle
    inputs of cbf_solve_dev for the R*C problems, in its layout (batch R*C, race-major, car-minor): obs_s, obs_ey [R*C,V,N+1], lap_off
    [R*C,V], n_obs [R*C] with V = C - 1; clear [R*C] (None with clear=False: not computed); obs_dims [R*C,V,2] with dims=True (the cars bring their own
    dimensions), else None.  n_pred: the columns of pred_s, pred_ey (None: N + 1; MixedWorkspace rolls out further)."""

    def __init__(self, desc, n_races, device, dims=False, clear=True, n_pred=None):
        N1, Cn = desc.N + 1, desc.n_cars
        Bn, V = n_races * Cn, Cn - 1
        f64 = dict(dtype=torch.float64, device=device)
        self.n_races = n_races
        self.pred_s = torch.zeros((n_races, Cn, n_pred or N1), **f64)
        self.pred_ey = torch.zeros((n_races, Cn, n_pred or N1), **f64)
        self.obs_s = torch.zeros((Bn, V, N1), **f64)
        self.obs_ey = torch.zeros((Bn, V, N1), **f64)
        self.lap_off = torch.zeros((Bn, V), **f64)
        self.n_obs = torch.zeros(Bn, dtype=torch.int32, device=device)
        self.obs_dims = torch.zeros((Bn, V, 2), **f64) if dims else None
        self.clear = torch.zeros(Bn, **f64) if clear else None


def _chk_field_ws(desc, ws, n_pred):
    """The arrays FieldWorkspace allocates, as field_prep_dev and mixed_prep_dev take them (n_pred: the roll-out's columns)."""
    R, Cn, N1 = ws.n_races, desc.n_cars, desc.N + 1
    Bn, V = R * Cn, Cn - 1
    for name, shape in (("pred_s", (R, Cn, n_pred)), ("pred_ey", (R, Cn, n_pred)), ("obs_s", (Bn, V, N1)), ("obs_ey", (Bn, V, N1)),
                        ("lap_off", (Bn, V)), ("obs_dims", (Bn, V, 2)), ("clear", (Bn,))):
        if getattr(ws, name) is not None:
            _chk(getattr(ws, name), torch.float64, shape, "ws." + name)
    _chk(ws.n_obs, torch.int32, (Bn,), "ws.n_obs")


def field_prep_dev(desc, track, xcurv, ws, car_dims=None):
    """crx_field_prep_dev (include/crx.h F1-F7): xcurv [R*C,6] (race-major, car-minor), track [n_seg,6], car_dims [R,C,2] (length, width
    per car) with a FieldWorkspace(dims=True), None with dims=False.  Writes ws and returns it."""
    _chk(track, torch.float64, (desc.n_seg, 6), "track")
    return _field_prep("crx_field_prep_dev", (_ptr(track),), desc, xcurv, ws, car_dims)


def field_prep_tracks_dev(desc, track_set, xcurv, ws, car_dims=None):
    """crx_field_prep_tracks_dev: field_prep_dev with race r on track track_set.race_track[r] of the RaceTrackSetDev `track_set`; desc's n_seg
    and lap_length are not used.  Writes ws and returns it."""
    return _field_prep("crx_field_prep_tracks_dev", _chk_race_track_set(track_set, ws.n_races), desc, xcurv, ws, car_dims)


def _field_prep(entry, track_args, desc, xcurv, ws, car_dims):
    """field_prep_dev / field_prep_tracks_dev: track_args is what the entry takes between n_races and xcurv."""
    R, Cn = ws.n_races, desc.n_cars
    _chk(xcurv, torch.float64, (R * Cn, 6), "xcurv")
    if (car_dims is None) != (ws.obs_dims is None):
        raise ValueError("car_dims goes with a FieldWorkspace(dims=True), no car_dims with dims=False")
    if car_dims is not None:
        _chk(car_dims, torch.float64, (R, Cn, 2), "car_dims")
    _chk_field_ws(desc, ws, desc.N + 1)
    _call(entry, C.byref(desc), C.c_int(R), *track_args, _ptr(xcurv), _ptr(car_dims), _ptr(ws.pred_s), _ptr(ws.pred_ey),
          _ptr(ws.obs_s), _ptr(ws.obs_ey), _ptr(ws.lap_off), _ptr(ws.n_obs), _ptr(ws.obs_dims), _ptr(ws.clear), _stream())
    return ws


class FieldTrafficWorkspace:
    """Outputs of field_traffic_dev for n_races races of desc.n_cars cars: every car's roll-out pred_s_car, pred_ey_car [R,C,N+1], and per
    ego the inputs of planner_scene_dev for the R*C scenarios (race-major, car-minor): veh_xcurv [R*C,V,6], pred_s, pred_ey [R*C,V,N+1],
    n_all [R*C] with V = C - 1.  With one car per race the per-ego arrays hold nothing; they are allocated with ONE zero slot (the kernel
    never writes it) so that a scene launch of n_all_max = 1 has arrays to take, and n_all is 0.  n_slots = max(V, 1)."""

    def __init__(self, desc, n_races, device):
        N1, Cn = desc.N + 1, desc.n_cars
        Bn, S = n_races * Cn, max(Cn - 1, 1)
        f64 = dict(dtype=torch.float64, device=device)
        self.n_races, self.n_slots = n_races, S
        self.pred_s_car = torch.zeros((n_races, Cn, N1), **f64)
        self.pred_ey_car = torch.zeros((n_races, Cn, N1), **f64)
        self.veh_xcurv = torch.zeros((Bn, S, 6), **f64)
        self.pred_s = torch.zeros((Bn, S, N1), **f64)
        self.pred_ey = torch.zeros((Bn, S, N1), **f64)
        self.n_all = torch.zeros(Bn, dtype=torch.int32, device=device)


def field_traffic_dev(desc, track, xcurv, ws):
    """crx_field_traffic_dev (include/crx.h "Field games", F1-F3, F6, G1-G3): xcurv [R*C,6] (race-major, car-minor), track [n_seg,6].
    Writes ws (a FieldTrafficWorkspace) and returns it."""
    R, Cn, N1 = ws.n_races, desc.n_cars, desc.N + 1
    Bn, S = R * Cn, max(Cn - 1, 1)
    _chk(track, torch.float64, (desc.n_seg, 6), "track")
    _chk(xcurv, torch.float64, (Bn, 6), "xcurv")
    for name, shape in (("pred_s_car", (R, Cn, N1)), ("pred_ey_car", (R, Cn, N1)), ("veh_xcurv", (Bn, S, 6)), ("pred_s", (Bn, S, N1)),
                        ("pred_ey", (Bn, S, N1))):
        _chk(getattr(ws, name), torch.float64, shape, "ws." + name)
    _chk(ws.n_all, torch.int32, (Bn,), "ws.n_all")
    _call("crx_field_traffic_dev", C.byref(desc), C.c_int(R), _ptr(track), _ptr(xcurv), _ptr(ws.pred_s_car), _ptr(ws.pred_ey_car),
          _ptr(ws.veh_xcurv), _ptr(ws.pred_s), _ptr(ws.pred_ey), _ptr(ws.n_all), _stream())
    return ws


class MixedWorkspace(FieldWorkspace):
    """Outputs of mixed_prep_dev for n_races races of desc.n_cars cars, batch R*C race-major and car-minor, V = C - 1: the roll-outs pred_s,
    pred_ey [R,C,NP+1] (NP = max(N, N_ilqr)); the NLP family in cbf_solve_dev's layout -- obs_s, obs_ey [R*C,V,N+1], lap_off [R*C,V], n_obs,
    m_nlp [R*C], obs_dims [R*C,V,2] with dims=True, else None; the iLQR family in ilqr_solve_dev's layout when desc.N_ilqr > 0, else None --
    il_obs_s, il_obs_ey [R*C,V,N_ilqr+1], il_lap_off [R*C,V], il_n_obs, m_ilqr [R*C]; clear [R*C] (None with clear=False)."""

    def __init__(self, desc, n_races, device, dims=False, clear=True):
        NI1, Cn = desc.N_ilqr + 1, desc.n_cars
        Bn, V = n_races * Cn, Cn - 1
        super().__init__(desc, n_races, device, dims=dims, clear=clear, n_pred=max(desc.N + 1, NI1))
        f64 = dict(dtype=torch.float64, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        self.m_nlp = torch.zeros(Bn, **i32)
        il = desc.N_ilqr > 0
        self.il_obs_s = torch.zeros((Bn, V, NI1), **f64) if il else None
        self.il_obs_ey = torch.zeros((Bn, V, NI1), **f64) if il else None
        self.il_lap_off = torch.zeros((Bn, V), **f64) if il else None
        self.il_n_obs = torch.zeros(Bn, **i32) if il else None
        self.m_ilqr = torch.zeros(Bn, **i32) if il else None


def mixed_prep_dev(desc, track, xcurv, policy, ws, car_dims=None):
    """crx_mixed_prep_dev (include/crx.h "Mixed fields"): xcurv [R*C,6] (race-major, car-minor), track [n_seg,6], policy int32 [R*C] of
    abi.POLICY_* codes, car_dims [R,C,2] with a MixedWorkspace(dims=True), None with dims=False.  Writes ws and returns it."""
    _chk(track, torch.float64, (desc.n_seg, 6), "track")
    return _mixed_prep("crx_mixed_prep_dev", (_ptr(track),), desc, xcurv, policy, ws, car_dims)


def mixed_prep_tracks_dev(desc, track_set, xcurv, policy, ws, car_dims=None):
    """crx_mixed_prep_tracks_dev: mixed_prep_dev with race r on track track_set.race_track[r] of the RaceTrackSetDev `track_set`; desc's
    n_seg and lap_length are not used.  Writes ws and returns it."""
    return _mixed_prep("crx_mixed_prep_tracks_dev", _chk_race_track_set(track_set, ws.n_races), desc, xcurv, policy, ws, car_dims)


def _mixed_prep(entry, track_args, desc, xcurv, policy, ws, car_dims):
    """mixed_prep_dev / mixed_prep_tracks_dev: track_args as in _field_prep."""
    R, Cn, NI1 = ws.n_races, desc.n_cars, desc.N_ilqr + 1
    Bn, V = R * Cn, Cn - 1
    _chk(xcurv, torch.float64, (Bn, 6), "xcurv")
    _chk(policy, torch.int32, (Bn,), "policy")
    if (car_dims is None) != (ws.obs_dims is None):
        raise ValueError("car_dims goes with a MixedWorkspace(dims=True), no car_dims with dims=False")
    if (desc.N_ilqr > 0) != (ws.m_ilqr is not None):
        raise ValueError("the workspace was built for another N_ilqr: its iLQR arrays go with desc.N_ilqr > 0")
    if car_dims is not None:
        _chk(car_dims, torch.float64, (R, Cn, 2), "car_dims")
    _chk_field_ws(desc, ws, max(desc.N + 1, NI1))
    for name, shape in (("il_obs_s", (Bn, V, NI1)), ("il_obs_ey", (Bn, V, NI1)), ("il_lap_off", (Bn, V))):
        if getattr(ws, name) is not None:
            _chk(getattr(ws, name), torch.float64, shape, "ws." + name)
    for name in ("m_nlp", "il_n_obs", "m_ilqr"):
        if getattr(ws, name) is not None:
            _chk(getattr(ws, name), torch.int32, (Bn,), "ws." + name)
    _call(entry, C.byref(desc), C.c_int(R), *track_args, _ptr(xcurv), _ptr(policy), _ptr(car_dims), _ptr(ws.pred_s), _ptr(ws.pred_ey),
          _ptr(ws.obs_s), _ptr(ws.obs_ey), _ptr(ws.lap_off), _ptr(ws.n_obs), _ptr(ws.obs_dims), _ptr(ws.m_nlp), _ptr(ws.il_obs_s), _ptr(ws.il_obs_ey),
          _ptr(ws.il_lap_off), _ptr(ws.il_n_obs), _ptr(ws.m_ilqr), _ptr(ws.clear), _stream())
    return ws


def mixed_commit_dev(policy, x, u, ctrl_status, pid=None, lqr=None, nlp=None, ilqr=None):
    """crx_mixed_commit_dev: u [B,2] and ctrl_status int32 [B] from each car's own law; policy int32 [B], x [B,6] the state the step starts
    from.  The families, each a pair or None (its cars then apply zero and report CRX_SKIPPED): pid = (vt, eyt) [B] each; lqr = (K [B,2,6],
    xt [B,6]); nlp = (U [B,N,2], status int32 [B]) of cbf_solve_dev; ilqr = (U [B,N_ilqr,2], status) of ilqr_solve_dev."""
    Bn = x.shape[0]
    _chk(policy, torch.int32, (Bn,), "policy")
    _chk(x, torch.float64, (Bn, 6), "x")
    _chk(u, torch.float64, (Bn, 2), "u")
    _chk(ctrl_status, torch.int32, (Bn,), "ctrl_status")
    vt, eyt = pid if pid is not None else (None, None)
    K, xt = lqr if lqr is not None else (None, None)
    Un, sn = nlp if nlp is not None else (None, None)
    Ui, si = ilqr if ilqr is not None else (None, None)
    if pid is not None:
        _chk(vt, torch.float64, (Bn,), "pid vt")
        _chk(eyt, torch.float64, (Bn,), "pid eyt")
    if lqr is not None:
        _chk(K, torch.float64, (Bn, 2, 6), "lqr K")
        _chk(xt, torch.float64, (Bn, 6), "lqr xt")
    strides = []
    for name, U, st in (("nlp", Un, sn), ("ilqr", Ui, si)):
        if U is not None:
            if U.dim() != 3 or U.shape[1] < 1:
                raise ValueError("%s U: expected [B,N,2]" % name)
            _chk(U, torch.float64, (Bn, U.shape[1], 2), name + " U")
            _chk(st, torch.int32, (Bn,), name + " status")
        strides.append(0 if U is None else 2 * U.shape[1])
    _call("crx_mixed_commit_dev", C.c_int(Bn), _ptr(policy), _ptr(x), _ptr(vt), _ptr(eyt), _ptr(K), _ptr(xt), _ptr(Un), C.c_int(strides[0]), _ptr(sn),
          _ptr(Ui), C.c_int(strides[1]), _ptr(si), _ptr(u), _ptr(ctrl_status), _stream())
    return u


class RaceStatsWorkspace:
    """State of race_stats_dev for `batch` cars (include/crx.h "Race statistics"): stat_i [STATS_NI, batch] int32 and stat_d
    [STATS_ND + n_opp_max, batch] float64, field-major, and every field as a named view of them: n_samples, nonfinite_step, off_step,
    off_samples, contact_step, contact_samples, n_laps, laps_prev, passes, passed, flag_samples [batch]; lap_step [8, batch];
    min_clear, ey_max, sum_ey2, sum_dv2 [batch]; ds_prev [n_opp_max, batch].  sum_i / sum_d: the records of the last summary."""

    def __init__(self, desc, batch, device):
        self.batch = batch
        self.stat_i = torch.zeros((abi.STATS_NI, batch), dtype=torch.int32, device=device)
        self.stat_d = torch.zeros((abi.STATS_ND + desc.n_opp_max, batch), dtype=torch.float64, device=device)
        for name, row in abi.STATS_I.items():
            setattr(self, name, self.stat_i[row:row + abi.CRX_STATS_MAX_LAPS] if name == "lap_step" else self.stat_i[row])
        for name, row in abi.STATS_D.items():
            setattr(self, name, self.stat_d[row:] if name == "ds_prev" else self.stat_d[row])
        self.sum_i = self.sum_d = None

    def fields(self):
        """name -> view, every field."""
        return {name: getattr(self, name) for name in list(abi.STATS_I) + list(abi.STATS_D)}


def _stats_ws(desc, ws, laps):
    Bn = ws.batch
    _chk(ws.stat_i, torch.int32, (abi.STATS_NI, Bn), "ws.stat_i")
    _chk(ws.stat_d, torch.float64, (abi.STATS_ND + desc.n_opp_max, Bn), "ws.stat_d")
    if laps is not None:
        _chk(laps, torch.int32, (Bn,), "laps")
    return Bn


def race_stats_reset_dev(desc, laps, ws):
    """crx_race_stats_reset_dev: every field of ws at its reset value, laps_prev = laps [batch] int32."""
    Bn = _stats_ws(desc, ws, laps)
    _call("crx_race_stats_reset_dev", C.byref(desc), Bn, _ptr(laps), _ptr(ws.stat_i), _ptr(ws.stat_d), _stream())
    return ws


def race_stats_dev(desc, sample, t, xcurv, laps, ws, car_s0=None, car_v=None, car_ey=None, n_opp=None, car_dims=None, xt=None, flag=None):
    """crx_race_stats_dev (include/crx.h S1-S4): one sample of every car, ONE launch.  xcurv [batch,6], laps [batch] int32; scripted mode
    (desc.n_cars == 0): car_s0, car_v, car_ey [batch, n_opp_max] at the clock t, n_opp [batch] int32 optional; field mode: car_dims
    [batch / n_cars, n_cars, 2] optional; xt [batch,6] and flag [batch] int32 optional.  Updates ws in place and returns it."""
    return _race_stats("crx_race_stats_dev", (), desc, sample, t, xcurv, laps, ws, car_s0, car_v, car_ey, n_opp, car_dims, xt, flag)


def race_stats_laps_dev(desc, sample, t, xcurv, laps, ws, car_s0=None, car_v=None, car_ey=None, n_opp=None, car_dims=None, xt=None, flag=None,
                        lap_length=None):
    """crx_race_stats_laps_dev: race_stats_dev with car b folded by lap_length[b] ([batch] float64 on the device; desc.lap_length is not
    used): the cars of a launch on tracks of their own."""
    if lap_length is None:
        raise ValueError("race_stats_laps_dev: lap_length [batch] is required (race_stats_dev takes the descriptor's one lap length)")
    _chk(lap_length, torch.float64, (ws.batch,), "lap_length")
    return _race_stats("crx_race_stats_laps_dev", (_ptr(lap_length),), desc, sample, t, xcurv, laps, ws, car_s0, car_v, car_ey, n_opp, car_dims, xt,
                       flag)


def _race_stats(entry, lap_args, desc, sample, t, xcurv, laps, ws, car_s0, car_v, car_ey, n_opp, car_dims, xt, flag):
    """race_stats_dev / race_stats_laps_dev: lap_args is what the entry takes between t and xcurv."""
    Bn, V = _stats_ws(desc, ws, laps), desc.n_opp_max
    _chk(xcurv, torch.float64, (Bn, 6), "xcurv")
    for name, a in (("car_s0", car_s0), ("car_v", car_v), ("car_ey", car_ey)):
        if a is not None:
            _chk(a, torch.float64, (Bn, V), name)
    for name, a in (("n_opp", n_opp), ("flag", flag)):
        if a is not None:
            _chk(a, torch.int32, (Bn,), name)
    if car_dims is not None:
        _chk(car_dims, torch.float64, (Bn // max(desc.n_cars, 1), max(desc.n_cars, 1), 2), "car_dims")
    if xt is not None:
        _chk(xt, torch.float64, (Bn, 6), "xt")
    _call(entry, C.byref(desc), Bn, int(sample), float(t), *lap_args, _ptr(xcurv), _ptr(laps), _ptr(car_s0), _ptr(car_v), _ptr(car_ey),
          _ptr(n_opp), _ptr(car_dims), _ptr(xt), _ptr(flag), _ptr(ws.stat_i), _ptr(ws.stat_d), _stream())
    return ws


def race_stats_summary_dev(desc, ws, group=None, n_groups=1):
    """crx_race_stats_summary_dev: the cars of ws reduced to one record per group (group [batch] int32 in [0, n_groups); None: one group).
    Writes ws.sum_i [G, STATS_SUM_NI] int64 and ws.sum_d [G, STATS_SUM_ND] float64 (abi.stats_summary_record names a row) and returns them."""
    Bn = _stats_ws(desc, ws, None)
    G = int(n_groups) if group is not None else 1
    if group is not None:
        _chk(group, torch.int32, (Bn,), "group")
    if ws.sum_i is None or ws.sum_i.shape[0] != max(G, 1):
        ws.sum_i = torch.zeros((max(G, 1), abi.STATS_SUM_NI), dtype=torch.int64, device=ws.stat_i.device)
        ws.sum_d = torch.zeros((max(G, 1), abi.STATS_SUM_ND), dtype=torch.float64, device=ws.stat_i.device)
    _call("crx_race_stats_summary_dev", C.byref(desc), Bn, _ptr(group), G, _ptr(ws.stat_i), _ptr(ws.stat_d), _ptr(ws.sum_i), _ptr(ws.sum_d),
          _stream())
    return ws.sum_i, ws.sum_d


def plant_step_wrap_dev(desc, track, xglob, xcurv, u, u_stride, xglob_next, xcurv_next, laps, noise_z=None, params=None):
    """crx_plant_step_wrap_dev: plant step + lap bookkeeping; `u` may be a strided view's base tensor (u_stride doubles
    between vehicles, e.g. the U output of cbf_solve_dev with u_stride = 2 N).  noise_z [B,3]: standard-normal draws for the
    reference's bounded process noise (utils/base.py:929-939; crx_plant_step_noise_dev), None = zero noise.  params [B,10]: one
    BicycleDynamicsParam set per vehicle (abi.plant_params; crx_plant_step_params_dev), None = desc's ten values for every vehicle."""
    Bn = xglob.shape[0]
    _chk(track, torch.float64, (desc.n_seg, 6), "track")
    _chk(xglob, torch.float64, (Bn, 6), "xglob")
    _chk(xcurv, torch.float64, (Bn, 6), "xcurv")
    _chk(xglob_next, torch.float64, (Bn, 6), "xglob_next")
    _chk(xcurv_next, torch.float64, (Bn, 6), "xcurv_next")
    _chk(laps, torch.int32, (Bn,), "laps")
    if not u.is_cuda or u.dtype != torch.float64 or not u.is_contiguous() or u.numel() < (Bn - 1) * u_stride + 2:
        raise ValueError("u: expected a contiguous cuda float64 tensor holding %d inputs at stride %d" % (Bn, u_stride))
    if noise_z is not None:
        _chk(noise_z, torch.float64, (Bn, 3), "noise_z")
    if params is not None:
        _chk(params, torch.float64, (Bn, 10), "params")
        _call("crx_plant_step_params_dev", C.byref(desc), C.c_int(Bn), _ptr(track), _ptr(xglob), _ptr(xcurv), _ptr(u), C.c_int(u_stride),
              _ptr(noise_z), _ptr(params), _ptr(xglob_next), _ptr(xcurv_next), _ptr(laps), _stream())
        return
    _call("crx_plant_step_noise_dev", C.byref(desc), C.c_int(Bn), _ptr(track), _ptr(xglob), _ptr(xcurv), _ptr(u),
          C.c_int(u_stride), _ptr(noise_z), _ptr(xglob_next), _ptr(xcurv_next), _ptr(laps), _stream())


class TrackSetDev:
    """A track set (abi.track_set) on a device, with every car's track: what the plant's `tracks` wrappers take.  track_id [B] int32,
    host array or tensor.  car_lap [B]: lap_length[track_id], the cars' own lap lengths.  Ids are checked here, once, on the host side of
    whatever they came from; the kernel gives a car whose id is out of range non-finite states."""

    def __init__(self, tracks, track_id, device):
        dev = torch.device(device)
        self.host = tracks
        self.n_tracks, self.seg_stride = tracks.n_tracks, tracks.seg_stride
        self.tracks = torch.as_tensor(tracks.tracks, dtype=torch.float64).to(dev).contiguous()
        self.n_seg = torch.as_tensor(tracks.n_seg, dtype=torch.int32).to(dev).contiguous()
        self.lap_length = torch.as_tensor(tracks.lap_length, dtype=torch.float64).to(dev).contiguous()
        tid = track_id if torch.is_tensor(track_id) else torch.as_tensor(track_id)
        if tid.dim() != 1 or tid.dtype.is_floating_point:
            raise ValueError("track_id: expected an integer [B] array, got %s %s" % (tid.dtype, tuple(tid.shape)))
        if tid.numel() and (int(tid.min()) < 0 or int(tid.max()) >= self.n_tracks):
            raise ValueError("track_id: values outside [0, %d)" % self.n_tracks)
        self.track_id = tid.to(dtype=torch.int32, device=dev).contiguous()
        self.car_lap = self.lap_length[self.track_id.long()].contiguous()


class RaceTrackSetDev(TrackSetDev):
    """A track set on a device with one track per RACE of n_cars cars, for the field families: race_track [R] int32, host array or tensor.
    track_id [R * n_cars] = race_track.repeat_interleave(n_cars) is what the plant's `tracks` wrappers take (all cars of a race share its
    track), car_lap [R * n_cars] the cars' own lap lengths (race_stats_laps_dev).  Ids are checked here, once, on the host side; the kernels
    give a race whose id is out of range non-finite predictions and no obstacles."""

    def __init__(self, tracks, race_track, n_cars, device):
        rt = race_track if torch.is_tensor(race_track) else torch.as_tensor(race_track)
        if rt.dim() != 1 or rt.dtype.is_floating_point or rt.dtype == torch.bool:
            raise ValueError("race_track: expected an integer [R] array, got %s %s" % (rt.dtype, tuple(rt.shape)))
        if rt.numel() and (int(rt.min()) < 0 or int(rt.max()) >= tracks.n_tracks):
            raise ValueError("race_track: values outside [0, %d)" % tracks.n_tracks)
        rt = rt.to(dtype=torch.int32, device=torch.device(device)).contiguous()
        super().__init__(tracks, rt.repeat_interleave(int(n_cars)), device)
        self.race_track, self.n_cars = rt, int(n_cars)


def _chk_race_track_set(ts, R):
    _chk(ts.tracks, torch.float64, (ts.n_tracks, ts.seg_stride, 6), "tracks")
    _chk(ts.n_seg, torch.int32, (ts.n_tracks,), "n_seg")
    _chk(ts.lap_length, torch.float64, (ts.n_tracks,), "lap_length")
    _chk(ts.race_track, torch.int32, (R,), "race_track")
    return C.c_int(ts.n_tracks), C.c_int(ts.seg_stride), _ptr(ts.tracks), _ptr(ts.n_seg), _ptr(ts.lap_length), _ptr(ts.race_track)


def _chk_track_set(ts, Bn):
    _chk(ts.tracks, torch.float64, (ts.n_tracks, ts.seg_stride, 6), "tracks")
    _chk(ts.n_seg, torch.int32, (ts.n_tracks,), "n_seg")
    _chk(ts.lap_length, torch.float64, (ts.n_tracks,), "lap_length")
    _chk(ts.track_id, torch.int32, (Bn,), "track_id")
    return C.c_int(ts.n_tracks), C.c_int(ts.seg_stride), _ptr(ts.tracks), _ptr(ts.n_seg), _ptr(ts.lap_length), _ptr(ts.track_id)


def plant_step_tracks_dev(desc, tracks, xglob, xcurv, u, xglob_next=None, xcurv_next=None, params=None):
    """crx_plant_step_tracks_plain_dev: plant_step_dev with vehicle b on track tracks.track_id[b] of the TrackSetDev `tracks`; returns
    (xglob_next, xcurv_next) (allocated unless given)."""
    Bn = xglob.shape[0]
    set_args = _chk_track_set(tracks, Bn)
    _chk(xglob, torch.float64, (Bn, 6), "xglob")
    _chk(xcurv, torch.float64, (Bn, 6), "xcurv")
    _chk(u, torch.float64, (Bn, 2), "u")
    if params is not None:
        _chk(params, torch.float64, (Bn, 10), "params")
    xglob_next = xglob_next if xglob_next is not None else torch.empty_like(xglob)
    xcurv_next = xcurv_next if xcurv_next is not None else torch.empty_like(xcurv)
    _call("crx_plant_step_tracks_plain_dev", C.byref(desc), C.c_int(Bn), *set_args, _ptr(xglob), _ptr(xcurv), _ptr(u), _ptr(params),
          _ptr(xglob_next), _ptr(xcurv_next), _stream())
    return xglob_next, xcurv_next


def plant_step_tracks_wrap_dev(desc, tracks, xglob, xcurv, u, u_stride, xglob_next, xcurv_next, laps, noise_z=None, params=None):
    """crx_plant_step_tracks_dev: plant_step_wrap_dev with vehicle b on track tracks.track_id[b] of the TrackSetDev `tracks`, its lap
    bookkeeping with that track's lap length.  laps None: no lap counters."""
    Bn = xglob.shape[0]
    set_args = _chk_track_set(tracks, Bn)
    _chk(xglob, torch.float64, (Bn, 6), "xglob")
    _chk(xcurv, torch.float64, (Bn, 6), "xcurv")
    _chk(xglob_next, torch.float64, (Bn, 6), "xglob_next")
    _chk(xcurv_next, torch.float64, (Bn, 6), "xcurv_next")
    if laps is not None:
        _chk(laps, torch.int32, (Bn,), "laps")
    if not u.is_cuda or u.dtype != torch.float64 or not u.is_contiguous() or u.numel() < (Bn - 1) * u_stride + 2:
        raise ValueError("u: expected a contiguous cuda float64 tensor holding %d inputs at stride %d" % (Bn, u_stride))
    if noise_z is not None:
        _chk(noise_z, torch.float64, (Bn, 3), "noise_z")
    if params is not None:
        _chk(params, torch.float64, (Bn, 10), "params")
    _call("crx_plant_step_tracks_dev", C.byref(desc), C.c_int(Bn), *set_args, _ptr(xglob), _ptr(xcurv), _ptr(u), C.c_int(u_stride),
          _ptr(noise_z), _ptr(params), _ptr(xglob_next), _ptr(xcurv_next), _ptr(laps), _stream())


def cbf_prep_laps_dev(N, lap_length, t, dt, xcurv, car_s0, car_v, car_ey, obs_s, obs_ey, lap_off, n_obs, safety_time=2.0):
    """crx_cbf_prep_laps_dev: cbf_prep_dev with race b folded and offset by lap_length[b] ([B] float64 on the device)."""
    Bn, V = car_s0.shape
    _chk(lap_length, torch.float64, (Bn,), "lap_length")
    _chk(xcurv, torch.float64, (Bn, 6), "xcurv")
    for name, a in (("car_s0", car_s0), ("car_v", car_v), ("car_ey", car_ey), ("lap_off", lap_off)):
        _chk(a, torch.float64, (Bn, V), name)
    _chk(obs_s, torch.float64, (Bn, V, N + 1), "obs_s")
    _chk(obs_ey, torch.float64, (Bn, V, N + 1), "obs_ey")
    _chk(n_obs, torch.int32, (Bn,), "n_obs")
    _call("crx_cbf_prep_laps_dev", C.c_int(N), C.c_int(V), _ptr(lap_length), C.c_double(t), C.c_double(dt),
          C.c_double(safety_time), C.c_int(Bn), _ptr(xcurv), _ptr(car_s0), _ptr(car_v), _ptr(car_ey), _ptr(obs_s),
          _ptr(obs_ey), _ptr(lap_off), _ptr(n_obs), _stream())


class LmpcPrepWorkspace:
    """Outputs of lmpc_prep_dev = the model and safe-set inputs of lmpc_solve_dev (same layout)."""

    def __init__(self, desc, batch, device):
        N, M = desc.N, desc.n_ss_per_lap * desc.n_ss_laps
        f64 = dict(dtype=torch.float64, device=device)
        # A, B, C are in/out: the kernel leaves the three regression rows of a singular stage (status 1) and everything of a
        # masked-out race untouched, so they start defined (zeros), never as uninitialised memory that could reach the QP
        self.A = torch.zeros((batch, N, 36), **f64)
        self.B = torch.zeros((batch, N, 12), **f64)
        self.C = torch.zeros((batch, N, 6), **f64)
        self.ss = torch.zeros((batch, 6, M), **f64)
        self.qfun = torch.zeros((batch, M), **f64)
        self.status = torch.zeros(batch, dtype=torch.int32, device=device)


def lmpc_prep_dev(desc, ss_xcurv, u_ss, qfun, time_ss, it, x, lin_points, lin_input, track, from_plan, ws=None, active=None):
    """crx_lmpc_prep_dev: the N stage models and the safe-set selection of every race (of the races with active != 0:
    crx_lmpc_prep_masked_dev)."""
    N, P, L, Bn = desc.N, desc.n_points, desc.n_laps, x.shape[0]
    _chk(ss_xcurv, torch.float64, (Bn, L, P, 6), "ss_xcurv")
    _chk(u_ss, torch.float64, (Bn, L, P, 2), "u_ss")
    _chk(qfun, torch.float64, (Bn, L, P), "qfun")
    _chk(time_ss, torch.int32, (Bn, L), "time_ss")
    _chk(it, torch.int32, (Bn,), "iter")
    _chk(x, torch.float64, (Bn, 6), "x")
    _chk(lin_points, torch.float64, (Bn, N + 1, 6), "lin_points")
    _chk(lin_input, torch.float64, (Bn, N, 2), "lin_input")
    _chk(track, torch.float64, (desc.n_seg, 6), "track")
    ws = ws or LmpcPrepWorkspace(desc, Bn, x.device)
    if active is not None:
        _chk(active, torch.int32, (Bn,), "active")
    _call("crx_lmpc_prep_masked_dev", C.byref(desc), C.c_int(Bn), _ptr(active) if active is not None else None, _ptr(ss_xcurv), _ptr(u_ss),
          _ptr(qfun), _ptr(time_ss), _ptr(it), _ptr(x),
          _ptr(lin_points), _ptr(lin_input), C.c_int(int(bool(from_plan))), _ptr(track), _ptr(ws.A), _ptr(ws.B), _ptr(ws.C),
          _ptr(ws.ss), _ptr(ws.qfun), _ptr(ws.status), _stream())
    return ws


def lmpc_addpoint_dev(desc, ss_xcurv, u_ss, time_ss, it, step, x, u, u_stride):
    """crx_lmpc_addpoint_dev: LMPCRacingGame.add_point for every race (in place)."""
    Bn, P, L = x.shape[0], desc.n_points, desc.n_laps
    _chk(ss_xcurv, torch.float64, (Bn, L, P, 6), "ss_xcurv")
    _chk(u_ss, torch.float64, (Bn, L, P, 2), "u_ss")
    _chk(time_ss, torch.int32, (Bn, L), "time_ss")
    _chk(it, torch.int32, (Bn,), "iter")
    _chk(step, torch.int32, (Bn,), "step")
    _chk(x, torch.float64, (Bn, 6), "x")
    if not u.is_cuda or u.dtype != torch.float64 or not u.is_contiguous() or u.numel() < (Bn - 1) * u_stride + 2:
        raise ValueError("u: expected a contiguous cuda float64 tensor holding %d inputs at stride %d" % (Bn, u_stride))
    _call("crx_lmpc_addpoint_dev", C.byref(desc), C.c_int(Bn), _ptr(ss_xcurv), _ptr(u_ss), _ptr(time_ss), _ptr(it), _ptr(step),
          _ptr(x), _ptr(u), C.c_int(u_stride), _stream())


def lmpc_addtraj_dev(desc, crossed, log_x, log_u, n_log, ss_xcurv, u_ss, qfun, time_ss, it, step, x, status):
    """crx_lmpc_addtraj_dev: LMPCRacingGame.add_trajectory for the races with crossed != 0 (everything in place)."""
    Bn, P, L = x.shape[0], desc.n_points, desc.n_laps
    _chk(crossed, torch.int32, (Bn,), "crossed")
    _chk(log_x, torch.float64, (Bn, P, 6), "log_x")
    _chk(log_u, torch.float64, (Bn, P, 2), "log_u")
    _chk(n_log, torch.int32, (Bn,), "n_log")
    _chk(ss_xcurv, torch.float64, (Bn, L, P, 6), "ss_xcurv")
    _chk(u_ss, torch.float64, (Bn, L, P, 2), "u_ss")
    _chk(qfun, torch.float64, (Bn, L, P), "qfun")
    _chk(time_ss, torch.int32, (Bn, L), "time_ss")
    _chk(it, torch.int32, (Bn,), "iter")
    _chk(step, torch.int32, (Bn,), "step")
    _chk(x, torch.float64, (Bn, 6), "x")
    _chk(status, torch.int32, (Bn,), "status")
    _call("crx_lmpc_addtraj_dev", C.byref(desc), C.c_int(Bn), _ptr(crossed), _ptr(log_x), _ptr(log_u), _ptr(n_log), _ptr(ss_xcurv),
          _ptr(u_ss), _ptr(qfun), _ptr(time_ss), _ptr(it), _ptr(step), _ptr(x), _ptr(status), _stream())


class SceneWorkspace:
    def __init__(self, desc, n_scen, device):
        N1, V = desc.N + 1, desc.n_veh_max
        f64 = dict(dtype=torch.float64, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        self.n_veh, self.overflow = torch.empty(n_scen, **i32), torch.empty(n_scen, **i32)
        self.order = torch.empty((n_scen, V), **i32)
        self.veh_info = torch.empty((n_scen, V, 3), **f64)
        self.max_dv = torch.empty(n_scen, **f64)
        self.obs_s, self.obs_ey = torch.empty((n_scen, V, N1), **f64), torch.empty((n_scen, V, N1), **f64)


def planner_scene_dev(desc, ego_xcurv, n_all, veh_xcurv, pred_s, pred_ey, ws=None):
    """crx_planner_scene_dev: interest test, partial sort, veh_infos, max_delta_v, predictions in sorted order."""
    N1, VA, S = desc.N + 1, desc.n_all_max, ego_xcurv.shape[0]
    _chk(ego_xcurv, torch.float64, (S, 6), "ego_xcurv")
    _chk(n_all, torch.int32, (S,), "n_all")
    _chk(veh_xcurv, torch.float64, (S, VA, 6), "veh_xcurv")
    _chk(pred_s, torch.float64, (S, VA, N1), "pred_s")
    _chk(pred_ey, torch.float64, (S, VA, N1), "pred_ey")
    ws = ws or SceneWorkspace(desc, S, ego_xcurv.device)
    _call("crx_planner_scene_dev", C.byref(desc), C.c_int(S), _ptr(ego_xcurv), _ptr(n_all), _ptr(veh_xcurv), _ptr(pred_s), _ptr(pred_ey),
          _ptr(ws.n_veh), _ptr(ws.overflow), _ptr(ws.order), _ptr(ws.veh_info), _ptr(ws.max_dv), _ptr(ws.obs_s), _ptr(ws.obs_ey), _stream())
    return ws


def planner_plan_dev(desc, sdesc, x0, bez_s, bez_ey, ey_lb, ey_ub, n_veh, obs_s, obs_ey, old_flag, ws, sws, active=None, models=None):
    """crx_planner_plan_dev: all region QPs of every scenario + the selection, on one stream (with `active`, int32
    [n_scen]: crx_planner_plan_masked_dev, the QPs of the scenarios with 0 are skipped).  models (a PlannerModels of n_scen models with
    regions = n_veh_max + 1): crx_planner_plan_models_dev, the region QPs of scenario i on model i (desc.A, desc.B are ignored)."""
    S, N, V = n_veh.shape[0], desc.N, sdesc.n_veh_max
    R = V + 1
    _chk(x0, torch.float64, (S * R, 6), "x0")
    _chk(bez_s, torch.float64, (S * R, N + 1), "bez_s")
    _chk(bez_ey, torch.float64, (S * R, N + 1), "bez_ey")
    _chk(ey_lb, torch.float64, (S * R, N), "ey_lb")
    _chk(ey_ub, torch.float64, (S * R,), "ey_ub")
    _chk(n_veh, torch.int32, (S,), "n_veh")
    _chk(obs_s, torch.float64, (S, V, N + 1), "obs_s")
    _chk(obs_ey, torch.float64, (S, V, N + 1), "obs_ey")
    _chk(old_flag, torch.int32, (S,), "old_flag")
    _chk(ws.X, torch.float64, (S * R, N + 1, 6), "ws.X")
    _chk(ws.U, torch.float64, (S * R, N, 2), "ws.U")
    for name in ("cost", "kkt"):
        _chk(getattr(ws, name), torch.float64, (S * R,), "ws." + name)
    for name in ("status", "iters"):
        _chk(getattr(ws, name), torch.int32, (S * R,), "ws." + name)
    _chk(sws.flag, torch.int32, (S,), "sws.flag")
    _chk(sws.sel_cost, torch.float64, (S, R), "sws.sel_cost")
    _chk(sws.best_X, torch.float64, (S, N + 1, 6), "sws.best_X")
    if active is not None:
        _chk(active, torch.int32, (S,), "active")
    if models is not None:
        m = _planner_models(models, desc, S * R)
        _call("crx_planner_plan_models_dev", C.byref(desc), C.byref(sdesc), C.c_int(S), _ptr(active), _ptr(x0), _ptr(m.A), _ptr(m.B), _ptr(m.reach),
              _ptr(bez_s), _ptr(bez_ey), _ptr(ey_lb), _ptr(ey_ub), _ptr(n_veh), _ptr(obs_s), _ptr(obs_ey), _ptr(old_flag), _ptr(ws.X), _ptr(ws.U),
              _ptr(ws.cost), _ptr(ws.status), _ptr(ws.kkt), _ptr(ws.iters), _ptr(sws.flag), _ptr(sws.sel_cost), _ptr(sws.best_X), _stream())
        return
    _call("crx_planner_plan_masked_dev", C.byref(desc), C.byref(sdesc), C.c_int(S), _ptr(active), _ptr(x0), _ptr(bez_s), _ptr(bez_ey), _ptr(ey_lb), _ptr(ey_ub),
          _ptr(n_veh), _ptr(obs_s), _ptr(obs_ey), _ptr(old_flag), _ptr(ws.X), _ptr(ws.U), _ptr(ws.cost), _ptr(ws.status), _ptr(ws.kkt),
          _ptr(ws.iters), _ptr(sws.flag), _ptr(sws.sel_cost), _ptr(sws.best_X), _stream())


class PathPlanWorkspace:
    """Outputs of path_prep_dev (opt .. span: the inputs of the path QPs, same layout) and of path_plan_dev (the rest).  E, kkt and target
    are what a skipped scenario leaves untouched: they start as NaN."""

    def __init__(self, desc, n_scen, device):
        N1, Bn = desc.N + 1, n_scen * (desc.n_veh_max + 1)
        f64 = dict(dtype=torch.float64, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        self.opt, self.bez, self.lb, self.ub = (torch.empty((Bn, N1), **f64) for _ in range(4))
        self.e0, self.eN, self.span = torch.empty(Bn, **f64), torch.empty(Bn, **f64), torch.empty(n_scen, **f64)
        self.qp_active = torch.empty(Bn, **i32)
        self.E = torch.full((Bn, N1), float("nan"), **f64)
        self.cost, self.kkt = torch.empty(Bn, **f64), torch.full((Bn,), float("nan"), **f64)
        self.status, self.iters = torch.empty(Bn, **i32), torch.empty(Bn, **i32)
        self.flag, self.plan_status = torch.empty(n_scen, **i32), torch.empty(n_scen, **i32)
        self.target = torch.full((n_scen, N1, 6), float("nan"), **f64)


def _path_inputs(desc, x_wrapped, x_raw, n_veh, order, veh_xcurv, max_dv, obs_ey, opt_s, opt_ey):
    N, V, VA, T, S = desc.N, desc.n_veh_max, desc.n_all_max, desc.n_opt, x_wrapped.shape[0]
    _chk(x_wrapped, torch.float64, (S, 6), "x_wrapped")
    _chk(x_raw, torch.float64, (S, 6), "x_raw")
    _chk(n_veh, torch.int32, (S,), "n_veh")
    _chk(order, torch.int32, (S, V), "order")
    _chk(veh_xcurv, torch.float64, (S, VA, 6), "veh_xcurv")
    _chk(max_dv, torch.float64, (S,), "max_dv")
    _chk(obs_ey, torch.float64, (S, V, N + 1), "obs_ey")
    _chk(opt_s, torch.float64, (T,), "opt_s")
    _chk(opt_ey, torch.float64, (T,), "opt_ey")
    return S, [_ptr(a) for a in (x_wrapped, x_raw, n_veh, order, veh_xcurv, max_dv, obs_ey, opt_s, opt_ey)]


def _path_ws(ws, desc, S, device):
    ws = ws or PathPlanWorkspace(desc, S, device)
    N1, Bn = desc.N + 1, S * (desc.n_veh_max + 1)
    for name in ("opt", "bez", "lb", "ub", "E"):
        _chk(getattr(ws, name), torch.float64, (Bn, N1), "ws." + name)
    for name in ("e0", "eN", "cost", "kkt"):
        _chk(getattr(ws, name), torch.float64, (Bn,), "ws." + name)
    for name in ("qp_active", "status", "iters"):
        _chk(getattr(ws, name), torch.int32, (Bn,), "ws." + name)
    _chk(ws.span, torch.float64, (S,), "ws.span")
    _chk(ws.flag, torch.int32, (S,), "ws.flag")
    _chk(ws.plan_status, torch.int32, (S,), "ws.plan_status")
    _chk(ws.target, torch.float64, (S, N1, 6), "ws.target")
    return ws


def path_prep_dev(desc, x_wrapped, x_raw, n_veh, order, veh_xcurv, max_dv, obs_ey, opt_s, opt_ey, ws=None):
    """crx_path_prep_dev (include/crx.h P1-P6): from the outputs of planner_scene_dev to ws.opt .. ws.span, the inputs of path_solve's
    QPs for every region of every scenario.  A scenario without vehicles keeps what the workspace held."""
    S, ins = _path_inputs(desc, x_wrapped, x_raw, n_veh, order, veh_xcurv, max_dv, obs_ey, opt_s, opt_ey)
    ws = _path_ws(ws, desc, S, x_wrapped.device)
    _call("crx_path_prep_dev", C.byref(desc), C.c_int(S), *ins, _ptr(ws.opt), _ptr(ws.bez), _ptr(ws.lb), _ptr(ws.ub), _ptr(ws.e0), _ptr(ws.eN),
          _ptr(ws.span), _stream())
    return ws


def path_solve_dev(qdesc, ws):
    """crx_path_solve_dev on a PathPlanWorkspace: EVERY region QP of ws.opt .. ws.eN (path_prep_dev's outputs) into ws.E, ws.cost,
    ws.status, ws.kkt, ws.iters -- the unmasked launch the fused step's middle stage is compared with."""
    Bn, N1 = ws.opt.shape
    if qdesc.N + 1 != N1:
        raise ValueError("path_solve_dev: the workspace was made for N = %d, the descriptor says %d" % (N1 - 1, qdesc.N))
    _call("crx_path_solve_dev", C.byref(qdesc), C.c_int(Bn), _ptr(ws.opt), _ptr(ws.bez), _ptr(ws.lb), _ptr(ws.ub), _ptr(ws.e0), _ptr(ws.eN),
          _ptr(ws.E), _ptr(ws.cost), _ptr(ws.status), _ptr(ws.kkt), _ptr(ws.iters), _stream())
    return ws


def path_plan_dev(desc, qdesc, x_wrapped, x_raw, n_veh, order, veh_xcurv, max_dv, obs_ey, opt_s, opt_ey, opt_vx, ws=None, active=None):
    """crx_path_plan_dev (include/crx.h P1-P8): prep, the region QPs and the selection with its target, three launches on the current
    stream.  active int32 [n_scen]: scenarios with 0 -- and those without vehicles -- are not planned (regions CRX_SKIPPED with cost inf,
    ws.flag -1, ws.plan_status CRX_SKIPPED, ws.target untouched)."""
    S, ins = _path_inputs(desc, x_wrapped, x_raw, n_veh, order, veh_xcurv, max_dv, obs_ey, opt_s, opt_ey)
    _chk(opt_vx, torch.float64, (desc.n_opt,), "opt_vx")
    if active is not None:
        _chk(active, torch.int32, (S,), "active")
    ws = _path_ws(ws, desc, S, x_wrapped.device)
    _call("crx_path_plan_dev", C.byref(desc), C.byref(qdesc), C.c_int(S), _ptr(active), *ins, _ptr(opt_vx), _ptr(ws.opt), _ptr(ws.bez), _ptr(ws.lb),
          _ptr(ws.ub), _ptr(ws.e0), _ptr(ws.eN), _ptr(ws.span), _ptr(ws.qp_active), _ptr(ws.E), _ptr(ws.cost), _ptr(ws.status), _ptr(ws.kkt),
          _ptr(ws.iters), _ptr(ws.flag), _ptr(ws.target), _ptr(ws.plan_status), _stream())
    return ws


def track_prep_dev(N, V, lap_length, x, n_veh, obs_s_in, obs_ey_in, traj, xt, obs_s, obs_ey, lap_off, n_obs, safety_time=2.0, dt_ref=0.1):
    """crx_track_prep_dev: per-stage targets and obstacle arrays of the tracking NLP from the planner's outputs."""
    Bn = x.shape[0]
    _chk(x, torch.float64, (Bn, 6), "x")
    _chk(n_veh, torch.int32, (Bn,), "n_veh")
    for name, a in (("obs_s_in", obs_s_in), ("obs_ey_in", obs_ey_in), ("obs_s", obs_s), ("obs_ey", obs_ey)):
        _chk(a, torch.float64, (Bn, V, N + 1), name)
    _chk(traj, torch.float64, (Bn, N + 1, 6), "traj")
    _chk(xt, torch.float64, (Bn, N + 1, 6), "xt")
    _chk(lap_off, torch.float64, (Bn, V), "lap_off")
    _chk(n_obs, torch.int32, (Bn,), "n_obs")
    _call("crx_track_prep_dev", C.c_int(N), C.c_int(V), C.c_double(lap_length), C.c_double(safety_time), C.c_double(dt_ref), C.c_int(Bn),
          _ptr(x), _ptr(n_veh), _ptr(obs_s_in), _ptr(obs_ey_in), _ptr(traj), _ptr(xt), _ptr(obs_s), _ptr(obs_ey), _ptr(lap_off), _ptr(n_obs),
          _stream())


# ---- device-resident racing-game loop: bookkeeping between the solver launches (include/crx.h crx_game_*) ----------------------
def game_traffic_dev(N, lap_length, t, dt, car_s0, car_v, car_ey, veh_xcurv, pred_s, pred_ey):
    Bn, VA = car_s0.shape
    for name, a in (("car_s0", car_s0), ("car_v", car_v), ("car_ey", car_ey)):
        _chk(a, torch.float64, (Bn, VA), name)
    _chk(veh_xcurv, torch.float64, (Bn, VA, 6), "veh_xcurv")
    _chk(pred_s, torch.float64, (Bn, VA, N + 1), "pred_s")
    _chk(pred_ey, torch.float64, (Bn, VA, N + 1), "pred_ey")
    _call("crx_game_traffic_dev", C.c_int(N), C.c_int(Bn), C.c_int(VA), C.c_double(lap_length), C.c_double(t), C.c_double(dt), _ptr(car_s0),
          _ptr(car_v), _ptr(car_ey), _ptr(veh_xcurv), _ptr(pred_s), _ptr(pred_ey), _stream())


def game_masks_dev(n_veh, m_overtake, m_lmpc, overflow=None, overflow_seen=None):
    Bn = n_veh.shape[0]
    for name, a in (("n_veh", n_veh), ("m_overtake", m_overtake), ("m_lmpc", m_lmpc)) + ((("overflow", overflow), ("overflow_seen", overflow_seen)) if overflow is not None else ()):
        _chk(a, torch.int32, (Bn,), name)
    _call("crx_game_masks_dev", C.c_int(Bn), _ptr(n_veh), _ptr(overflow), _ptr(m_overtake), _ptr(m_lmpc), _ptr(overflow_seen), _stream())


def game_commit_dev(N, Np, overtake, U_track, X_lmpc, U_lmpc, flag, u, u_old, u_prev, lin_points, lin_input, step_no, addpoint_step, old_flag):
    Bn = u.shape[0]
    _chk(X_lmpc, torch.float64, (Bn, N + 1, 6), "X_lmpc")
    _chk(U_lmpc, torch.float64, (Bn, N, 2), "U_lmpc")
    for name, a in (("u", u), ("u_old", u_old), ("u_prev", u_prev)):
        _chk(a, torch.float64, (Bn, 2), name)
    _chk(lin_points, torch.float64, (Bn, N + 1, 6), "lin_points")
    _chk(lin_input, torch.float64, (Bn, N, 2), "lin_input")
    _chk(step_no, torch.int32, (Bn,), "step_no")
    _chk(addpoint_step, torch.int32, (Bn,), "addpoint_step")
    if overtake is not None:
        _chk(overtake, torch.int32, (Bn,), "overtake")
        _chk(U_track, torch.float64, (Bn, Np, 2), "U_track")
        _chk(flag, torch.int32, (Bn,), "flag")
        _chk(old_flag, torch.int32, (Bn,), "old_flag")
    _call("crx_game_commit_dev", C.c_int(N), C.c_int(Np), C.c_int(Bn), _ptr(overtake), _ptr(U_track), _ptr(X_lmpc), _ptr(U_lmpc), _ptr(flag),
          _ptr(u), _ptr(u_old), _ptr(u_prev), _ptr(lin_points), _ptr(lin_input), _ptr(step_no), _ptr(addpoint_step), _ptr(old_flag), _stream())


def game_log_dev(lap_length, xcurv, u, laps, laps_prev, log_x, log_u, n_log, crossed):
    Bn, P = log_x.shape[0], log_x.shape[1]
    _chk(xcurv, torch.float64, (Bn, 6), "xcurv")
    _chk(u, torch.float64, (Bn, 2), "u")
    for name, a in (("laps", laps), ("laps_prev", laps_prev), ("n_log", n_log), ("crossed", crossed)):
        _chk(a, torch.int32, (Bn,), name)
    _chk(log_x, torch.float64, (Bn, P, 6), "log_x")
    _chk(log_u, torch.float64, (Bn, P, 2), "log_u")
    _call("crx_game_log_dev", C.c_int(Bn), C.c_int(P), C.c_double(lap_length), _ptr(xcurv), _ptr(u), _ptr(laps), _ptr(laps_prev), _ptr(log_x),
          _ptr(log_u), _ptr(n_log), _ptr(crossed), _stream())


# ---- seed laps: each car's PID lap and MPC-LTI lap into its own safe set (include/crx.h "Seed laps", S1-S6) ------------------------------
def seed_commit_dev(N, phase, vt, eyt, x, U_mpc, mpc_status, seed_status, u):
    """crx_seed_commit_dev, after the solver launch and before the plant: u [B,2] <- control.pid of x (phase 0), U_mpc[:, 0] (phase 1; a
    solver status other than converged sets bit CRX_SEED_MPC_FAILED of seed_status) or zero (phase >= 2)."""
    Bn = u.shape[0]
    for name, a in (("phase", phase), ("mpc_status", mpc_status), ("seed_status", seed_status)):
        _chk(a, torch.int32, (Bn,), name)
    _chk(vt, torch.float64, (Bn,), "vt")
    _chk(eyt, torch.float64, (Bn,), "eyt")
    _chk(x, torch.float64, (Bn, 6), "x")
    _chk(U_mpc, torch.float64, (Bn, N, 2), "U_mpc")
    _chk(u, torch.float64, (Bn, 2), "u")
    _call("crx_seed_commit_dev", C.c_int(N), C.c_int(Bn), _ptr(phase), _ptr(vt), _ptr(eyt), _ptr(x), _ptr(U_mpc), _ptr(mpc_status),
          _ptr(seed_status), _ptr(u), _stream())


def seed_log_dev(lap_length, xcurv_prev, xglob_prev, xcurv, xglob, u, laps, laps_prev, log_x, log_u, n_log, crossed, phase, seed_status, m_mpc):
    """crx_seed_log_dev, after the plant and before lmpc_addtraj_dev: a car in phase >= 2 is put back to (xcurv_prev, xglob_prev, laps_prev);
    a driving car logs the step as game_log_dev does and its phase moves on; m_mpc <- (phase == 1)."""
    Bn, P = log_x.shape[0], log_x.shape[1]
    for name, a in (("xcurv_prev", xcurv_prev), ("xglob_prev", xglob_prev), ("xcurv", xcurv), ("xglob", xglob)):
        _chk(a, torch.float64, (Bn, 6), name)
    _chk(u, torch.float64, (Bn, 2), "u")
    for name, a in (("laps", laps), ("laps_prev", laps_prev), ("n_log", n_log), ("crossed", crossed), ("phase", phase),
                    ("seed_status", seed_status), ("m_mpc", m_mpc)):
        _chk(a, torch.int32, (Bn,), name)
    _chk(log_x, torch.float64, (Bn, P, 6), "log_x")
    _chk(log_u, torch.float64, (Bn, P, 2), "log_u")
    if xcurv_prev.data_ptr() == xcurv.data_ptr() or xglob_prev.data_ptr() == xglob.data_ptr():
        raise ValueError("seed_log_dev: the plant's two state pairs must be different tensors")
    _call("crx_seed_log_dev", C.c_int(Bn), C.c_int(P), C.c_double(lap_length), _ptr(xcurv_prev), _ptr(xglob_prev), _ptr(xcurv), _ptr(xglob),
          _ptr(u), _ptr(laps), _ptr(laps_prev), _ptr(log_x), _ptr(log_u), _ptr(n_log), _ptr(crossed), _ptr(phase), _ptr(seed_status),
          _ptr(m_mpc), _stream())
