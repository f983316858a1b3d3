"""One LTI model per problem for the MPC-CBF / tracking NLP kernels (crx_cbf_solve_models*, GPU box only).

The reference of every parity test is the oracle as it stands: it takes the model in the descriptor, so problem b is one batch-1
orc.cbf_solve with abi.cbf_desc(..., A_b, B_b).  Tolerances and the status / iteration rules are the project's own -- DEFAULT,
_assert_same_verdicts and _cmp of tests/test_gpu_parity.py, imported, with the budgets that file gives the same draws.
Model family (tools/lqr_bench.py): rng = default_rng(seed); per problem A0 (1 + s z66), then B0 (1 + s z62)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import conftest
from test_gpu_parity import DEFAULT, _assert_same_verdicts, _cmp

pytestmark = pytest.mark.gpu
KEYS = ("X", "U", "sigma", "cost", "status", "kkt", "iters")
IN = ("x0", "xt", "obs_s", "obs_ey", "lap_off", "n_obs")
CRX_SINGULAR, CRX_SKIPPED, CRX_ERR_ARG = 6, 4, -1
REACH_ROW = 25   # CRX_MAX_N + 1


@pytest.fixture(scope="module")
def gpu():
    import crx

    return crx.init(0)


def family(AB, n, s, seed):
    rng = np.random.default_rng(seed)
    mA, mB = np.empty((n, 6, 6)), np.empty((n, 6, 2))
    for b in range(n):
        mA[b] = AB[0] * (1 + s * rng.standard_normal((6, 6)))
        mB[b] = AB[1] * (1 + s * rng.standard_normal((6, 2)))
    return mA, mB


def copies(AB, n):
    return np.repeat(AB[0][None], n, axis=0), np.repeat(AB[1][None], n, axis=0)


@functools.lru_cache(maxsize=None)
def draw(case):
    """The draws of the issue's table: -> (inputs dict, descriptor keywords, seed)."""
    from crx import synth

    cfg4 = dict(alpha=0.6, margin=0.15, Q=(10.0, 0, 0, 5.0, 0, 50.0), per_stage_target=True)
    if case == "a":
        p, kw, seed = synth.cfg2_mpccbf(64, N=12, seed=7, safe_start=False), {}, 7
    elif case == "b":
        p, kw, seed = synth.cfg2_mpccbf(64, N=10, seed=7, safe_start=False), {}, 7
    elif case == "c":
        p, kw, seed = synth.cfg4_tracking_cbf(48, N=20, seed=8), cfg4, 8
    elif case == "d":   # zero obstacle slots (the mpc_lti form)
        p, kw, seed = synth.cfg2_mpccbf(32, N=10, seed=9), {}, 9
        z = np.zeros((32, 0, 11))
        p.update(obs_s=z, obs_ey=z, lap_off=np.zeros((32, 0)), n_obs=np.zeros(32, np.int32))
    elif case == "e":   # a run-time horizon: the general unit
        p, kw, seed = synth.cfg4_tracking_cbf(16, N=7, seed=10, n_obs=2), cfg4, 10
    elif case == "f":   # five slots: the generic six-slot instantiation
        p, kw, seed = synth.cfg4_tracking_cbf(16, N=12, seed=11, n_obs=5), cfg4, 11
    else:               # "g": another exponent
        p, kw, seed = synth.cfg2_mpccbf(16, N=12, seed=12, safe_start=False), dict(degree=4), 12
    if "alpha" not in kw:
        kw = dict(kw, alpha=p["alpha"], margin=p["margin"])
    p["n_obs"] = np.ascontiguousarray(p["n_obs"], dtype=np.int32)
    return p, kw, seed


def desc(case, AB, A=None, B=None, **opts):
    from crx import abi

    p, kw, _ = draw(case)
    d = abi.cbf_desc(p["N"], p["obs_s"].shape[1], AB[0] if A is None else A, AB[1] if B is None else B, **kw)
    for k, v in opts.items():
        setattr(d.opts, k, v)
    return d


def args_of(p, sl=slice(None)):
    return tuple(p[k][sl] for k in IN)


_ORACLE = {}


def oracle_per_model(orc, AB, case, s, **opts):
    """Problem b of the draw on model b of the family: one oracle call of batch 1 each, computed once per (case, s, options)."""
    key = (case, s, tuple(sorted(opts.items())))
    if key not in _ORACLE:
        p, _, seed = draw(case)
        n = len(p["x0"])
        mA, mB = family(AB, n, s, seed)
        rows = [orc.cbf_solve(desc(case, AB, mA[b], mB[b], **opts), *args_of(p, slice(b, b + 1))) for b in range(n)]
        r = {k: np.concatenate([x[k] for x in rows]) for k in KEYS}
        for v in r.values():
            v.setflags(write=False)
        _ORACLE[key] = r
    return _ORACLE[key]


def assert_bits(a, b, keys=KEYS, rows=slice(None), tag=""):
    for k in keys:
        np.testing.assert_array_equal(np.asarray(a[k])[rows], np.asarray(b[k])[rows], err_msg="%s %s" % (tag, k))


def reach_numpy(A, B, delta_max, a_max, row, N):
    """reach_bound of csrc/crx_api.hip, operation by operation in float64."""
    gain = np.zeros(REACH_ROW)
    w = np.zeros(6)
    w[row] = 1.0
    acc = 0.0
    for j in range(1, N + 1):
        v0 = v1 = 0.0
        for i in range(6):
            v0 = v0 + w[i] * B[i, 0]
            v1 = v1 + w[i] * B[i, 1]
        acc = acc + (abs(v0) * delta_max + abs(v1) * a_max)
        gain[j] = acc
        wn = np.zeros(6)
        for a in range(6):
            for i in range(6):
                wn[a] = wn[a] + w[i] * A[i, a]
        w = wn
    return gain


def _dev():
    import torch

    return torch.device("cuda", 0)


def _t(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a).to(_dev())


def _ws_dict(ws):
    import torch

    torch.cuda.synchronize()
    return {k: getattr(ws, k).cpu().numpy() for k in KEYS}


@pytest.mark.parametrize("N", [10, 12, 20, 24])
def test_1_reach_table_is_the_host_table_bit_for_bit(gpu, AB, N):
    from crx import abi, torch_api

    mA, mB = family(AB, 64, 5e-2, 100 + N)
    mA, mB = np.concatenate([mA, AB[0][None]]), np.concatenate([mB, AB[1][None]])
    d = abi.cbf_desc(N, 1, *AB, delta_max=0.5, a_max=1.0)
    m = torch_api.CbfModels(d, _t(mA), _t(mB))
    got = m.reach.cpu().numpy()
    want = np.array([[reach_numpy(mA[b], mB[b], d.delta_max, d.a_max, r, N) for r in (4, 5)] for b in range(65)])
    assert got.shape == (65, 2, REACH_ROW)
    np.testing.assert_array_equal(got, want)
    assert (got[:, :, 1:N + 1] > 0).all() and (got[:, :, N + 1:] == 0).all() and (got[:, :, 0] == 0).all()


@pytest.mark.parametrize("case", list("abcdefg"))
def test_2_copies_of_the_shipped_model_are_the_shared_launch(gpu, AB, case):
    """One case per translation unit / instantiation class; through the device entry (CbfModels) and the host-pointer entry."""
    from crx import torch_api

    p, _, _ = draw(case)
    n = len(p["x0"])
    d = desc(case, AB)
    shared = gpu.cbf_solve(d, *args_of(p))
    print("copies %s: status counts %s, iterations %d..%d" % (case, np.bincount(shared["status"]).tolist(), shared["iters"].min(), shared["iters"].max()))
    assert (shared["status"] == 0).any()
    host = gpu.cbf_solve(d, *args_of(p), models=copies(AB, n))
    assert_bits(host, shared, tag=case + " host entry")
    a = [_t(p[k]) for k in IN]
    m = torch_api.CbfModels(d, *[_t(x) for x in copies(AB, n)])
    # (with zero obstacle slots CbfWorkspace still holds one slot of sigma, which no kernel writes: nothing to compare)
    keys = KEYS if d.n_obs_max else tuple(k for k in KEYS if k != "sigma")
    assert_bits(_ws_dict(torch_api.cbf_solve_dev(d, *a, models=m)), shared, keys=keys, tag=case + " device entry")
    assert_bits(_ws_dict(torch_api.cbf_solve_dev(d, *a)), shared, keys=keys, tag=case + " shared device entry")


def test_2b_copies_on_a_shape_the_shared_launch_runs_tuned_and_the_models_launch_general(gpu, AB):
    """Two obstacle slots at N = 12: the shared launch runs the tuned <2,12,6,12>, the models launch the general <2,12,6,0> (include/crx.h
    promises bit equality only within one instantiation class).  The same iteration through another instantiation: same verdicts and
    iteration counts under the project's rules, the same points to DEFAULT.  Whether the bits are equal is printed, not required."""
    from crx import abi, synth

    p = synth.cfg4_tracking_cbf(32, N=12, seed=14, n_obs=2)
    d = abi.cbf_desc(12, 2, *AB, alpha=0.6, margin=0.15, Q=(10.0, 0, 0, 5.0, 0, 50.0), per_stage_target=True)
    args = tuple(np.ascontiguousarray(p[k], dtype=np.int32 if k == "n_obs" else None) for k in IN)
    shared = gpu.cbf_solve(d, *args)
    own = gpu.cbf_solve(d, *args, models=copies(AB, 32))
    print("tuned against general, copies: bit-equal X %s, iteration counts differ on %d of 32, max|dX| %.3g" % (
        np.array_equal(shared["X"], own["X"]), (shared["iters"] != own["iters"]).sum(), np.abs(shared["X"] - own["X"]).max()))
    crashy = frozenset(np.nonzero((own["status"] != shared["status"]) | (own["iters"] != shared["iters"]))[0].tolist())
    _assert_same_verdicts("tuned against general", own, shared, restored=crashy, max_restored_verdict=2)
    assert len(crashy) <= 4, len(crashy)
    _cmp("tuned against general", own, shared, need_same_status=False, T=DEFAULT)


@pytest.mark.parametrize("s", [1e-3, 1e-2, 5e-2])
@pytest.mark.parametrize("case", list("acd"))
def test_3_distinct_models_against_the_oracle(gpu, orc, AB, case, s):
    """Verdicts by _assert_same_verdicts with the budgets tests/test_gpu_parity.py::test_synthetic_cbf_batches gives these draws: the
    problems the restoration phase touches (found as there: whatever changes on either side when it is switched off) are comparable
    by class of outcome only; X, U, cost of the pairs converged on both sides to DEFAULT; at least 90 % of the batch such pairs."""
    p, _, seed = draw(case)
    n = len(p["x0"])
    models = family(AB, n, s, seed)
    g0 = gpu.cbf_solve(desc(case, AB, restore_iters=-1), *args_of(p), models=models)
    g1 = gpu.cbf_solve(desc(case, AB), *args_of(p), models=models)
    o0, o1 = oracle_per_model(orc, AB, case, s, restore_iters=-1), oracle_per_model(orc, AB, case, s)
    touched = set()
    for r0, r1 in ((g0, g1), (o0, o1)):
        dx = np.abs(r0["X"] - r1["X"]).reshape(n, -1).max(axis=1) > 0
        touched |= set(np.nonzero((r0["status"] != r1["status"]) | (r0["iters"] != r1["iters"]) | dx)[0].tolist())
    both = (g1["status"] == 0) & (o1["status"] == 0)
    tag = "models %s s=%g" % (case, s)
    print("%s: converged gpu %d oracle %d both %d of %d, touched by restoration %d, iteration counts differ on %d" % (
        tag, (g1["status"] == 0).sum(), (o1["status"] == 0).sum(), both.sum(), n, len(touched), (g1["iters"] != o1["iters"]).sum()))
    _assert_same_verdicts(tag + " no restoration", g0, o0, max_other=1 if case == "a" else 0)
    _assert_same_verdicts(tag, g1, o1, restored=frozenset(touched), max_restored_verdict=max(2, len(touched) // 5))
    _cmp(tag, g1, o1, need_same_status=False, T=DEFAULT)
    assert both.sum() >= 0.9 * n, (tag, int(both.sum()))


def test_4_batch_independence(gpu, AB):
    from crx import torch_api

    p, _, seed = draw("a")
    n = len(p["x0"])
    mA, mB = family(AB, n, 1e-2, seed)
    d = desc("a", AB)
    a = [_t(p[k]) for k in IN]
    m = torch_api.CbfModels(d, _t(mA), _t(mB))
    full = _ws_dict(torch_api.cbf_solve_dev(d, *a, models=m))
    # under a random order
    order = _t(np.random.default_rng(3).permutation(n).astype(np.int32))
    assert_bits(_ws_dict(torch_api.cbf_solve_dev(d, *a, models=m, order=order)), full, tag="order")
    # at another offset
    sh = 5
    roll = lambda x: np.roll(x, sh, axis=0)   # noqa: E731
    mr = torch_api.CbfModels(d, _t(roll(mA)), _t(roll(mB)))
    rolled = _ws_dict(torch_api.cbf_solve_dev(d, *[_t(roll(p[k])) for k in IN], models=mr))
    assert_bits(rolled, {k: roll(v) for k, v in full.items()}, tag="offset")
    for b in (0, 3, 31, 63):
        # alone, at batch 1
        one = slice(b, b + 1)
        m1 = torch_api.CbfModels(d, _t(mA[one]), _t(mB[one]))
        assert_bits(_ws_dict(torch_api.cbf_solve_dev(d, *[_t(p[k][one]) for k in IN], models=m1)), {k: v[one] for k, v in full.items()},
                    tag="alone %d" % b)
        # with its neighbours masked out: they stay untouched
        act = np.zeros(n, np.int32)
        act[b] = 1
        ws = torch_api.CbfWorkspace(d, n, _dev())
        for k in ("X", "U", "sigma", "cost", "kkt"):
            getattr(ws, k).fill_(-7.0)
        r = _ws_dict(torch_api.cbf_solve_dev(d, *a, ws=ws, models=m, active=_t(act), order=order))
        assert_bits(r, full, rows=one, tag="masked %d" % b)
        off = act == 0
        assert (r["status"][off] == CRX_SKIPPED).all() and (r["iters"][off] == 0).all()
        for k in ("X", "U", "sigma", "cost", "kkt"):
            assert (r[k][off] == -7.0).all(), k


def test_5_non_finite_models_never_enter_the_iteration(gpu, AB):
    from crx import torch_api

    p, _, seed = draw("a")
    n = len(p["x0"])
    mA, mB = family(AB, n, 1e-2, seed)
    d = desc("a", AB)
    clean = gpu.cbf_solve(d, *args_of(p), models=(mA, mB))
    pA, pB = mA.copy(), mB.copy()
    pA[3, 2, 4] = np.nan
    pB[17, 5, 1] = np.inf
    bad = np.zeros(n, bool)
    bad[[3, 17]] = True
    a = [_t(p[k]) for k in IN]
    dev = _ws_dict(torch_api.cbf_solve_dev(d, *a, models=torch_api.CbfModels(d, _t(pA), _t(pB))))
    host = gpu.cbf_solve(d, *args_of(p), models=(pA, pB))
    for tag, r in (("device entry", dev), ("host entry", host)):
        assert (r["status"][bad] == CRX_SINGULAR).all() and (r["iters"][bad] == 0).all() and np.isinf(r["kkt"][bad]).all(), tag
        for k in ("X", "U", "sigma", "cost"):
            assert np.isnan(r[k][bad]).all(), (tag, k)
        assert_bits(r, clean, rows=~bad, tag=tag)


def test_6_mixed_null_model_pointers_are_an_argument_error(gpu, AB):
    import crx
    from crx import torch_api
    from crx.torch_api import _ptr, _stream

    p, _, _ = draw("b")
    n = len(p["x0"])
    d = desc("b", AB)
    a = [_t(p[k]) for k in IN]
    m = torch_api.CbfModels(d, *[_t(x) for x in copies(AB, n)])
    ws = torch_api.CbfWorkspace(d, n, _dev())
    L = crx.lib()

    def call(mA, mB, mR):
        return L.crx_cbf_solve_models_dev(C.byref(d), C.c_int(n), None, None, _ptr(a[0]), mA, mB, mR, _ptr(a[1]), _ptr(a[2]), _ptr(a[3]),
                                          _ptr(a[4]), _ptr(a[5]), None, _ptr(ws.X), _ptr(ws.U), _ptr(ws.sigma), _ptr(ws.cost),
                                          _ptr(ws.status), _ptr(ws.kkt), _ptr(ws.iters), _stream())

    A_, B_, R_ = _ptr(m.A), _ptr(m.B), _ptr(m.reach)
    for mix in ((A_, None, None), (None, B_, None), (None, None, R_), (A_, B_, None), (A_, None, R_), (None, B_, R_)):
        assert call(*mix) == CRX_ERR_ARG, mix
        assert b"model_A, model_B and model_reach" in L.crx_last_error()
    assert call(A_, B_, R_) == 0 and call(None, None, None) == 0
    # the host-pointer entry: A and B go together
    x = [np.ascontiguousarray(p[k]) for k in IN]
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)   # noqa: E731
    out = {k: np.zeros_like(v) for k, v in _ws_dict(ws).items()}
    mA, mB = copies(AB, n)
    for hA, hB in ((ptr(mA), None), (None, ptr(mB))):
        rc = L.crx_cbf_solve_models(C.byref(d), C.c_int(n), ptr(x[0]), hA, hB, ptr(x[1]), ptr(x[2]), ptr(x[3]), ptr(x[4]), ptr(x[5]), None,
                                    ptr(out["X"]), ptr(out["U"]), ptr(out["sigma"]), ptr(out["cost"]), ptr(out["status"]), ptr(out["kkt"]),
                                    ptr(out["iters"]))
        assert rc == CRX_ERR_ARG and b"model_A and model_B go together" in L.crx_last_error()


def _races(track, AB, n, models=None, seed=13):
    """n races from the start line at vt, one scripted car inside the controller's window ahead of each ego."""
    from crx import montecarlo

    rng = np.random.default_rng(seed)
    x0 = np.zeros((n, 6))
    x0[:, 0] = 0.8
    s0 = rng.uniform(0.6, 1.5, (n, 1))
    v = rng.uniform(0.1, 0.4, (n, 1))
    ey = rng.choice([-0.3, -0.1, 0.1, 0.3], (n, 1))
    r = montecarlo.MpccbfRaces(track.point_and_tangent, track.lap_length, track.width, AB[0], AB[1], x0, x0, s0, v, ey, vt=0.8, N=10,
                               models=models)
    return r, x0


def _step0_against_oracle(r, x0, orc, mA, mB, tag, need_share):
    """Step 0 of every race (the inputs crx_cbf_prep_dev left on the device, the solve's outputs) against one oracle solve per car."""
    import torch
    from crx import abi

    torch.cuda.synchronize()
    ins = (x0, r.xt.cpu().numpy(), r.obs_s.cpu().numpy(), r.obs_e.cpu().numpy(), r.lap_off.cpu().numpy(), r.n_obs.cpu().numpy())
    rg = {k: getattr(r.ws, k).cpu().numpy().copy() for k in KEYS}
    d = r.desc
    rows = []
    for b in range(len(x0)):
        if not (np.isfinite(mA[b]).all() and np.isfinite(mB[b]).all()):
            assert rg["status"][b] == CRX_SINGULAR
            rows.append({k: rg[k][b:b + 1] for k in KEYS})   # no oracle for a model that is not a model
            continue
        db = abi.cbf_desc(d.N, d.n_obs_max, mA[b], mB[b], alpha=d.alpha, margin=d.margin, ey_max=d.ey_max)
        rows.append(orc.cbf_solve(db, *[x[b:b + 1] for x in ins]))
    ro = {k: np.concatenate([x[k] for x in rows]) for k in KEYS}
    both = (rg["status"] == 0) & (ro["status"] == 0)
    # the rule of tests/test_gpu_parity.py::test_general_horizons_against_oracle, both halves.  First restore_iters = -1, where exact status /
    # iteration parity is defined: the same step-0 problems through the host-pointer entry on the same models against the oracle
    import crx

    n = len(x0)
    fin = np.array([np.isfinite(mA[b]).all() and np.isfinite(mB[b]).all() for b in range(n)])
    d0 = abi.cbf_desc(d.N, d.n_obs_max, d.A, d.B, alpha=d.alpha, margin=d.margin, ey_max=d.ey_max)
    d0.opts.restore_iters = -1
    g0 = crx.binding().cbf_solve(d0, *[x[fin] for x in ins], models=(mA[fin], mB[fin]))
    rows0 = []
    for b in np.nonzero(fin)[0]:
        db = abi.cbf_desc(d.N, d.n_obs_max, mA[b], mB[b], alpha=d.alpha, margin=d.margin, ey_max=d.ey_max)
        db.opts.restore_iters = -1
        rows0.append(orc.cbf_solve(db, *[x[b:b + 1] for x in ins]))
    o0 = {k: np.concatenate([x[k] for x in rows0]) for k in KEYS}
    # then the product defaults (crash path on): the problems that took it are comparable by class of outcome only, and they are few
    crashy = frozenset(np.nonzero((rg["status"] != ro["status"]) | (rg["iters"] != ro["iters"]))[0].tolist())
    print("%s: step 0 converged gpu %d oracle %d both %d of %d; without restoration status / iterations differ on %d, with it on %d" % (
        tag, (rg["status"] == 0).sum(), (ro["status"] == 0).sum(), both.sum(), n,
        ((g0["status"] != o0["status"]) | (g0["iters"] != o0["iters"])).sum(), len(crashy)))
    _assert_same_verdicts(tag + " no restoration", g0, o0, max_tol_edge=max(1, 6 * n // 256), max_other=max(1, 2 * n // 256) if n >= 128 else 0)
    _assert_same_verdicts(tag, rg, ro, restored=crashy, max_restored_verdict=max(2, n // 50))
    assert len(crashy) <= max(1, n // 8), (tag, len(crashy))
    if both.any():
        _cmp(tag, rg, ro, need_same_status=False, T=DEFAULT)
    if need_share is not None:
        assert both.sum() >= need_share * len(x0), (tag, int(both.sum()))
    return rg


def test_7_closed_loop(gpu, orc, AB):
    import scenarios
    import torch

    track = scenarios.make_track("l_shape", 1.0)
    n, steps = 64, 30
    plain, x0 = _races(track, AB, n)
    same, _ = _races(track, AB, n, models=copies(AB, n))
    for k in range(steps):
        plain.step()
        same.step()
        assert torch.equal(plain.xc, same.xc) and torch.equal(plain.u, same.u) and torch.equal(plain.ws.status, same.ws.status), k
    assert torch.isfinite(plain.xc).all()
    mA, mB = family(AB, n, 1e-2, 13)
    own, _ = _races(track, AB, n, models=(mA, mB))
    own.step()
    _step0_against_oracle(own, x0, orc, mA, mB, "races, family s=1e-2", need_share=0.9)


def test_8_the_chain_pid_laps_identify_races(gpu, orc):
    """pid_laps -> identify() -> MpccbfRaces(models=...) with the models never leaving the device.  The identified models are far from
    the shipped one (the oracle itself converges on few of the problems they pose): plumbing and agreement, not solver quality."""
    import torch
    from crx import montecarlo
    from utils import racing_env

    S = np.load(os.path.join(conftest.GOLDEN, "sysid.npz"))
    track = racing_env.ClosedTrack(S["track_spec"], track_width=1.0)
    n, T = 8, int(S["short/steps"])
    x0p = np.tile(S["short/x0"], (n, 1))
    z = np.repeat(S["short/z"][:, None, :], n, axis=1)
    vt = float(S["short/vt"]) * (1.0 + 0.05 * np.arange(n))
    laps = montecarlo.pid_laps(track.point_and_tangent, track.lap_length, x0p, x0p, T, vt=vt, noise_z=z)
    fit = laps.identify(float(S["short/lamb"]))
    assert fit.A.is_cuda and fit.B.is_cuda
    AB0 = (np.genfromtxt(os.path.join(conftest.ROOT, "data/sys/LTI/matrix_A.csv"), delimiter=","),
           np.genfromtxt(os.path.join(conftest.ROOT, "data/sys/LTI/matrix_B.csv"), delimiter=","))
    r, x0 = _races(track, AB0, n, models=(fit.A, fit.B))
    assert r.models.A.data_ptr() == fit.A.data_ptr() and r.models.B.data_ptr() == fit.B.data_ptr()   # held, not copied
    r.step()
    mA, mB = fit.A.cpu().numpy(), fit.B.cpu().numpy()
    assert (fit.status.cpu().numpy() == 0).all() and not np.array_equal(mA[0], mA[1])
    _step0_against_oracle(r, x0, orc, mA, mB, "chain", need_share=None)
    for k in range(1, 10):
        r.step()
        torch.cuda.synchronize()
        ok = (r.ws.status != CRX_SINGULAR).cpu().numpy()
        for name in ("X", "U", "cost"):
            assert np.isfinite(getattr(r.ws, name).cpu().numpy()[ok]).all(), (k, name)
        assert np.isfinite(r.xc.cpu().numpy()[ok]).all(), k
