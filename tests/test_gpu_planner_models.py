"""One LTI model per planner region QP (crx_planner_solve_models*, crx_planner_plan_models*, GameLaps(models=); GPU box only).

The reference of every parity test is the oracle as it stands: it takes the model in the descriptor, so scenario i is one
orc.planner_solve over its V + 1 regions with abi.planner_desc(N, A_i, B_i).  Tolerances and the status / iteration rules are the
project's own -- DEFAULT, _assert_same_verdicts and _cmp of tests/test_gpu_parity.py, imported.
Model family (tests/test_gpu_cbf_models.py): rng = default_rng(seed); per scenario A0 (1 + s z66), then B0 (1 + s z62).
Draws: a, b run the tuned N = 12 / 10 kernels on both sides; c (N = 7) the general kernel on both sides; d (N = 20) the general
kernel with models against the tuned one of the shared launch."""
import functools
import os

import numpy as np
import pytest

import conftest
from test_gpu_cbf_models import _dev, _t, assert_bits, copies, family
from test_gpu_parity import DEFAULT, _assert_same_verdicts, _cmp
from test_planner_models_cpu import CRX_MAX_N, planner_reach_numpy

pytestmark = pytest.mark.gpu
KEYS = ("X", "U", "cost", "status", "kkt", "iters")
SEL = ("flag", "sel_cost", "best_X")
QIN = ("x0", "bez_s", "bez_ey", "ey_lb", "ey_ub")
CRX_INFEASIBLE, CRX_SKIPPED, CRX_SINGULAR = 2, 4, 6
DRAWS = {"a": (32, 12, 21, 3), "b": (16, 10, 22, 3), "c": (16, 7, 23, 2), "d": (8, 20, 24, 3)}   # n_scen, N, seed, V
SCALES = (1e-3, 1e-2, 5e-2)


@pytest.fixture(scope="module")
def gpu():
    import crx

    return crx.init(0)


@functools.lru_cache(maxsize=None)
def draw(case):
    from crx import synth

    n, N, seed, V = DRAWS[case]
    p = synth.cfg3_planner(n, N=N, seed=seed, V=V)
    for k in QIN + ("obs_s", "obs_ey"):
        p[k] = np.ascontiguousarray(p[k], dtype=np.float64)
    return p


def descs(case, AB, **opts):
    from crx import abi

    p = draw(case)
    return abi.planner_desc(p["N"], *AB, opts=abi.default_opts(**opts) if opts else None), abi.select_desc(p["N"], p["V"], p["lap_length"])


def qargs(p, sl=slice(None)):
    return tuple(p[k][sl] for k in QIN)


def sargs(p, sl=slice(None)):
    return (np.ascontiguousarray(p["n_veh"][sl], dtype=np.int32), p["obs_s"][sl], p["obs_ey"][sl], np.ascontiguousarray(p["old_flag"][sl], dtype=np.int32))


def per_region(m, R):
    return np.repeat(m[0], R, axis=0), np.repeat(m[1], R, axis=0)


_ORACLE = {}


def oracle_per_model(orc, AB, case, s):
    """Scenario i of the draw on model i of the family: one oracle call over its regions, computed once per (case, s)."""
    from crx import abi

    if (case, s) not in _ORACLE:
        p = draw(case)
        n, N, seed, V = DRAWS[case]
        R = V + 1
        mA, mB = family(AB, n, s, seed)
        rows = [orc.planner_solve(abi.planner_desc(N, mA[i], mB[i]), *qargs(p, slice(i * R, (i + 1) * R))) for i in range(n)]
        r = {k: np.concatenate([np.asarray(x[k]) for x in rows]) for k in KEYS}
        for v in r.values():
            v.setflags(write=False)
        _ORACLE[case, s] = r
    return _ORACLE[case, s]


def against_oracle(tag, rg, ro):
    """The rules of tests/test_gpu_parity.py::test_synthetic_planner_batch_and_selection and ::test_reach_screen_changes_no_verdict."""
    print("%s: converged gpu %d oracle %d of %d, screened %d, iterations <= %d" % (
        tag, (rg["status"] == 0).sum(), (ro["status"] == 0).sum(), len(ro["status"]), ((rg["status"] == CRX_INFEASIBLE) & (rg["iters"] == 0)).sum(),
        rg["iters"].max()))
    _assert_same_verdicts(tag, rg, ro)
    _cmp(tag, rg, ro, need_same_status=False, T=DEFAULT)
    fb = rg["status"] != 0
    np.testing.assert_allclose(rg["X"][fb], ro["X"][fb], atol=1e-12, err_msg=tag)
    assert np.isinf(rg["cost"][fb]).all() and (rg["cost"][fb] > 0).all(), tag
    np.testing.assert_array_equal((rg["status"] == CRX_INFEASIBLE) & (rg["iters"] == 0), (ro["status"] == CRX_INFEASIBLE) & (ro["iters"] == 0), err_msg=tag)


def _ws(ws, sws=None):
    import torch

    torch.cuda.synchronize()
    r = {k: getattr(ws, k).cpu().numpy() for k in KEYS}
    if sws is not None:
        r.update({k: getattr(sws, k).cpu().numpy() for k in SEL})
    return r


def plan_dev(d, sd, p, models=None, active=None, sl=slice(None), fill=None):
    """planner_plan_dev on scenarios sl of the draw (models: per scenario, host arrays) -> host dict of the QP and selection outputs."""
    from crx import torch_api

    R = sd.n_veh_max + 1
    S = len(p["n_veh"][sl])
    q = slice(None) if sl == slice(None) else slice(sl.start * R, sl.stop * R)
    ws, sws = torch_api.PlannerWorkspace(d, S * R, _dev()), torch_api.SelectWorkspace(sd, S, _dev())
    if fill is not None:
        for k in ("X", "U", "cost", "kkt"):
            getattr(ws, k).fill_(fill)
    m = None if models is None else torch_api.PlannerModels(d, _t(models[0]), _t(models[1]), regions=R)
    torch_api.planner_plan_dev(d, sd, *[_t(x) for x in qargs(p, q)], *[_t(x) for x in sargs(p, sl)], ws, sws,
                               active=None if active is None else _t(active), models=m)
    return _ws(ws, sws)


@pytest.mark.parametrize("N", [7, 10, 12, 20, 24])
def test_1_reach_table(gpu, AB, N):
    """Copies of the shipped model: the table the library computes on the host for the descriptor (reach_bound of csrc/crx_api.hip, here in
    its numpy restatement: tests/test_planner_models_cpu.py pins that to matrix powers and to the oracle's screen; test 2 pins the device
    table to the host one through the screen's verdicts).  The family at s = 5e-2: the restatement, bit for bit.  Zeros for j >= N."""
    from crx import abi, torch_api

    mA, mB = family(AB, 64, 5e-2, 200 + N)
    mA, mB = np.concatenate([mA, AB[0][None]]), np.concatenate([mB, AB[1][None]])
    d = abi.planner_desc(N, *AB)
    m = torch_api.PlannerModels(d, _t(mA), _t(mB))
    assert m.A.data_ptr() != 0 and m.regions == 1
    got = m.reach.cpu().numpy()
    want = np.array([planner_reach_numpy(mA[b], mB[b], d.delta_max, d.a_max, N) for b in range(65)])
    assert got.shape == (65, CRX_MAX_N, 7)
    np.testing.assert_array_equal(got, want)
    assert not got[:, N:].any() and (got[:, 1:N, 6] > 0).all() and (got[:, 0, 6] == 0).all()
    # regions: scenario i's model and table repeated for its regions
    m3 = torch_api.PlannerModels(d, _t(mA), _t(mB), regions=3)
    assert m3.batch == 195
    np.testing.assert_array_equal(m3.reach.cpu().numpy(), np.repeat(want, 3, axis=0))
    np.testing.assert_array_equal(m3.A.cpu().numpy(), np.repeat(mA, 3, axis=0))


@pytest.mark.parametrize("case,opts", [("a", {}), ("a", dict(qp_method=1)), ("a", dict(reach_screen=0)), ("b", {}), ("c", {})])
def test_2_copies_of_the_shipped_model_are_the_shared_launch(gpu, AB, case, opts):
    """Same instantiation class on both sides: bit for bit, through the device entry, the host-pointer entry and the fused step."""
    from crx import torch_api

    p = draw(case)
    n, R = p["n_scen"], p["V"] + 1
    d, sd = descs(case, AB, **opts)
    shared = gpu.planner_solve(d, *qargs(p))
    print("copies %s %s: status counts %s, iterations <= %d" % (case, opts, np.bincount(shared["status"]).tolist(), shared["iters"].max()))
    assert (shared["status"] == 0).any() and (shared["status"] != 0).any()
    cp = copies(AB, n)
    assert_bits(gpu.planner_solve(d, *qargs(p), models=per_region(cp, R)), shared, keys=KEYS, tag=case + " host entry")
    m = torch_api.PlannerModels(d, _t(cp[0]), _t(cp[1]), regions=R)
    a = [_t(x) for x in qargs(p)]
    assert_bits(_ws(torch_api.planner_solve_dev(d, *a, models=m)), shared, keys=KEYS, tag=case + " device entry")
    assert_bits(_ws(torch_api.planner_solve_dev(d, *a)), shared, keys=KEYS, tag=case + " shared device entry")
    plan = gpu.planner_plan(d, sd, *qargs(p), *sargs(p))
    assert_bits(plan, shared, keys=KEYS, tag=case + " shared plan")
    assert_bits(gpu.planner_plan(d, sd, *qargs(p), *sargs(p), models=cp), plan, keys=KEYS + SEL, tag=case + " host plan")
    assert_bits(plan_dev(d, sd, p, models=cp), plan, keys=KEYS + SEL, tag=case + " device plan")
    assert_bits(plan_dev(d, sd, p), plan, keys=KEYS + SEL, tag=case + " shared device plan")


def test_2d_copies_tuned_against_general(gpu, AB):
    """N = 20: the shared launch runs the tuned <0,24,0,20>, the models launch the general <0,24,0,0> (include/crx.h promises bit equality only
    within one instantiation class).  Same verdicts under the project's rules, the same points to DEFAULT, through all three entries; the
    fused step selects among its own trajectories."""
    from crx import torch_api

    p = draw("d")
    n, R = p["n_scen"], p["V"] + 1
    d, sd = descs("d", AB)
    shared = gpu.planner_solve(d, *qargs(p))
    cp = copies(AB, n)
    m = torch_api.PlannerModels(d, _t(cp[0]), _t(cp[1]), regions=R)
    plan = gpu.planner_plan(d, sd, *qargs(p), *sargs(p), models=cp)
    for tag, own in (("host entry", gpu.planner_solve(d, *qargs(p), models=per_region(cp, R))),
                     ("device entry", _ws(torch_api.planner_solve_dev(d, *[_t(x) for x in qargs(p)], models=m))), ("host plan", plan),
                     ("device plan", plan_dev(d, sd, p, models=cp))):
        print("tuned against general, %s: bit-equal X %s, max|dX| %.3g" % (tag, np.array_equal(shared["X"], own["X"]), np.abs(shared["X"] - own["X"]).max()))
        _assert_same_verdicts("d " + tag, own, shared)
        _cmp("d " + tag, own, shared, need_same_status=False, T=DEFAULT)
        fb = own["status"] != 0
        np.testing.assert_allclose(own["X"][fb], shared["X"][fb], atol=1e-12)
    X = plan["X"].reshape(n, R, p["N"] + 1, 6)
    assert ((plan["flag"] >= 0) & (plan["flag"] < R)).all()
    np.testing.assert_array_equal(plan["best_X"], X[np.arange(n), plan["flag"]])


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("case", list("abcd"))
def test_3_distinct_models_against_the_oracle(gpu, orc, AB, case, s):
    p = draw(case)
    n, N, seed, V = DRAWS[case]
    d, sd = descs(case, AB)
    models = family(AB, n, s, seed)
    ro = oracle_per_model(orc, AB, case, s)
    tag = "models %s s=%g" % (case, s)
    host = gpu.planner_solve(d, *qargs(p), models=per_region(models, V + 1))
    against_oracle(tag + " host entry", host, ro)
    dev = plan_dev(d, sd, p, models=models)
    assert_bits(dev, host, keys=KEYS, tag=tag + " device plan = host entry")


def test_4_the_model_is_the_problems_own(gpu, orc, AB):
    """Draw a at s = 1e-3: every QP that converges both with its own model and through the shared launch moves by more than 1e-3 =
    2 DEFAULT["x"] in the cost-weighted states (on the oracle the smallest such move is 5.9e-3 against the shared model, 1.2e-2 against
    the neighbouring scenario's): a kernel that read the descriptor, or model b +- 1, would sit within DEFAULT of the wrong answer."""
    p = draw("a")
    n, N, seed, V = DRAWS["a"]
    R = V + 1
    d, _ = descs("a", AB)
    models = family(AB, n, 1e-3, seed)
    own = gpu.planner_solve(d, *qargs(p), models=per_region(models, R))
    shared = gpu.planner_solve(d, *qargs(p))
    nb = gpu.planner_solve(d, *qargs(p), models=per_region(tuple(np.roll(m, 1, axis=0) for m in models), R))
    assert 2 * DEFAULT["x"] == 1e-3
    for tag, other in (("shared", shared), ("neighbour", nb)):
        both = (own["status"] == 0) & (other["status"] == 0)
        dmin = np.abs(own["X"][both] - other["X"][both])[..., [0, 4, 5]].reshape(both.sum(), -1).max(axis=1).min()
        print("own model against %s: %d pairs, smallest move %.3g" % (tag, both.sum(), dmin))
        assert both.sum() >= 60 and dmin > 1e-3, (tag, int(both.sum()), dmin)


def test_5_batch_independence(gpu, AB):
    p = draw("a")
    n, N, seed, V = DRAWS["a"]
    R = V + 1
    d, sd = descs("a", AB)
    mA, mB = family(AB, n, 1e-2, seed)
    full = plan_dev(d, sd, p, models=(mA, mB))
    # the batch rolled by 5 scenarios
    sh = 5
    pr = dict(p)
    for k in QIN:
        pr[k] = np.roll(p[k], sh * R, axis=0)
    for k in ("n_veh", "obs_s", "obs_ey", "old_flag"):
        pr[k] = np.roll(p[k], sh, axis=0)
    rolled = plan_dev(d, sd, pr, models=(np.roll(mA, sh, axis=0), np.roll(mB, sh, axis=0)))
    assert_bits(rolled, {k: np.roll(v, sh * (1 if k in SEL else R), axis=0) for k, v in full.items()}, keys=KEYS + SEL, tag="rolled")
    # scenarios [3:9] alone
    part = plan_dev(d, sd, p, models=(mA[3:9], mB[3:9]), sl=slice(3, 9))
    assert_bits(part, {k: v[3:9] if k in SEL else v[3 * R:9 * R] for k, v in full.items()}, keys=KEYS + SEL, tag="alone")
    # every third scenario masked out: skipped, outputs untouched, the others unchanged
    act = (np.arange(n) % 3 != 1).astype(np.int32)
    r = plan_dev(d, sd, p, models=(mA, mB), active=act, fill=-7.0)
    on = act != 0
    onq = np.repeat(on, R)
    assert (r["status"][~onq] == CRX_SKIPPED).all() and (r["iters"][~onq] == 0).all()
    for k in ("X", "U", "cost", "kkt"):
        assert (r[k][~onq] == -7.0).all(), k
    assert_bits(r, full, keys=KEYS, rows=onq, tag="masked")
    assert_bits(r, full, keys=SEL, rows=on, tag="masked selection")
    # the per-problem mask of the solve entry
    from crx import torch_api

    actq = np.ascontiguousarray(np.repeat(act, R))
    m = torch_api.PlannerModels(d, _t(mA), _t(mB), regions=R)
    ws = torch_api.PlannerWorkspace(d, n * R, _dev())
    ws.X.fill_(-7.0)
    rs = _ws(torch_api.planner_solve_dev(d, *[_t(x) for x in qargs(p)], ws=ws, models=m, active=_t(actq)))
    assert (rs["status"][~onq] == CRX_SKIPPED).all() and (rs["X"][~onq] == -7.0).all()
    assert_bits(rs, full, keys=KEYS, rows=onq, tag="masked solve")


def test_6_non_finite_models_answer_with_the_fall_back(gpu, AB):
    from crx import torch_api

    p = draw("a")
    n, N, seed, V = DRAWS["a"]
    R = V + 1
    d, sd = descs("a", AB)
    mA, mB = family(AB, n, 1e-2, seed)
    clean = plan_dev(d, sd, p, models=(mA, mB))
    pA, pB = mA.copy(), mB.copy()
    pA[2, 2, 4] = np.nan
    pB[5, 5, 1] = np.inf
    bad = np.zeros(n, bool)
    bad[[2, 5]] = True
    badq = np.repeat(bad, R)
    # the fall-back of the same regions: what the shared launch writes when the region is forced infeasible (it needs x0 and the Bezier arrays only)
    forced = dict(p)
    forced["ey_ub"] = np.full_like(p["ey_ub"], -10.0)
    fb = gpu.planner_solve(d, *qargs(forced))
    assert (fb["status"] == CRX_INFEASIBLE).all() and (fb["iters"] == 0).all()
    dev = plan_dev(d, sd, p, models=(pA, pB))
    host = gpu.planner_plan(d, sd, *qargs(p), *sargs(p), models=(pA, pB))
    solve = gpu.planner_solve(d, *qargs(p), models=per_region((pA, pB), R))
    for tag, r in (("device plan", dev), ("host plan", host), ("host solve", solve)):
        assert (r["status"][badq] == CRX_SINGULAR).all() and (r["iters"][badq] == 0).all(), tag
        assert np.isinf(r["kkt"][badq]).all() and np.isinf(r["cost"][badq]).all() and (r["cost"][badq] > 0).all(), tag
        assert (r["U"][badq] == 0).all(), tag
        np.testing.assert_array_equal(r["X"][badq], fb["X"][badq], err_msg=tag)
        assert_bits(r, clean, keys=KEYS, rows=~badq, tag=tag)
        if "flag" in r:
            assert_bits(r, clean, keys=SEL, rows=~bad, tag=tag)
            assert ((r["flag"][bad] >= 0) & (r["flag"][bad] < R)).all() and np.isfinite(r["best_X"][bad]).all(), tag


# ---- the racing game -------------------------------------------------------------------------------------------------------------
def _game(AB, g, n, models=None, seed=41):
    """n races at the start of the reference's first learning-MPC lap, two scripted cars 1.0 and 2.2 m ahead of every ego: step 0 is the
    overtake branch for every race."""
    import helpers
    import scenarios
    from crx import montecarlo

    track = scenarios.make_track("l_shape", 1.0)
    opt = scenarios.table("optimal_traj", "xcurv_l_shape")
    _, ss, us, qf, time_ss, lin_points, lin_input = helpers.lmpc_lap_setup(g, track)
    rng = np.random.default_rng(seed)
    x0 = np.tile(g["lmpc/x"][0], (n, 1))
    xg0 = np.tile(g["lap1/xglob"][-1], (n, 1))
    x0[:, 0] += rng.uniform(-0.03, 0.03, n)
    xg0[:, 0] = x0[:, 0]
    s0 = x0[:, 4, None] + np.array([1.0, 2.2])[None]
    v = rng.uniform(0.3, 0.7, (n, 2))
    ey = rng.choice([-0.4, -0.2, 0.1, 0.3], (n, 2))
    tile = lambda a: np.tile(a[None], (n,) + (1,) * a.ndim)   # noqa: E731
    A, B = AB if AB is not None else (None, None)
    r = montecarlo.GameLaps(track.point_and_tangent, track.lap_length, track.width, A, B, opt, tile(ss), tile(us), tile(qf), tile(time_ss),
                            np.full(n, 2, dtype=np.int32), x0, xg0, tile(lin_points), tile(lin_input), s0, v, ey, models=models)
    return r, track


def _step0_regions(r):
    """What the region QPs of the step just taken read (crx_planner_prep_dev left it on the device) and wrote."""
    import torch

    torch.cuda.synchronize()
    ins = tuple(getattr(r.pws, k).cpu().numpy() for k in QIN)
    return ins, _ws(r.qws, r.selws)


def _regions_against_oracle(tag, orc, r, ins, rg, mA, mB, parity=True):
    from crx import abi

    R = r.V + 1
    rows = [orc.planner_solve(abi.planner_desc(r.Np, mA[b], mB[b]), *[x[b * R:(b + 1) * R] for x in ins]) for b in range(len(mA))]
    ro = {k: np.concatenate([np.asarray(x[k]) for x in rows]) for k in KEYS}
    if parity:
        against_oracle(tag, rg, ro)
    else:
        print("%s: converged gpu %d oracle %d of %d" % (tag, (rg["status"] == 0).sum(), (ro["status"] == 0).sum(), len(ro["status"])))
        np.testing.assert_array_equal(rg["status"] == 0, ro["status"] == 0, err_msg=tag)
    return ro


def test_7_game_laps(gpu, orc, AB, golden_racing_game):
    import torch

    n = 16
    plain, track = _game(AB, golden_racing_game, n)
    same, _ = _game(AB, golden_racing_game, n, models=copies(AB, n))
    plain.step()
    same.step()
    (pin, pq), (sin, sq) = _step0_regions(plain), _step0_regions(same)
    assert (plain.m_ot.cpu().numpy() == 1).all() and (same.m_ot.cpu().numpy() == 1).all()   # every race overtakes at step 0
    for a, b in zip(pin, sin):
        np.testing.assert_array_equal(a, b)
    assert (pq["status"] == 0).any()
    assert_bits(sq, pq, keys=KEYS + SEL, tag="copies, step 0 region QPs and selection")
    # the tracking NLP: two obstacle slots at N = 10 -- tuned when shared, the general kernel with models: no bit claim
    tk = ("X", "U", "sigma", "cost", "status", "kkt", "iters")
    tp, ts = ({k: getattr(x.tws, k).cpu().numpy() for k in tk} for x in (plain, same))
    print("copies, tracking NLP: status tuned %s general %s, max|dX| %.3g" % (tp["status"].tolist(), ts["status"].tolist(), np.abs(tp["X"] - ts["X"]).max()))
    _cmp("copies, tracking NLP", ts, tp, need_same_status=False, T=DEFAULT)
    for k in range(1, 30):
        same.step()
    torch.cuda.synchronize()
    xc = same.lm.xc.cpu().numpy()
    assert np.isfinite(xc).all() and np.isfinite(same.u.cpu().numpy()).all() and np.abs(xc[:, 5]).max() <= 1.3 * track.width
    # the family: every race's region QPs on ITS model, against the oracle race by race
    mA, mB = family(AB, n, 1e-2, 41)
    own, _ = _game(AB, golden_racing_game, n, models=(mA, mB))
    own.step()
    oin, oq = _step0_regions(own)
    assert (own.m_ot.cpu().numpy() == 1).all()
    _regions_against_oracle("game, family s=1e-2", orc, own, oin, oq, mA, mB)
    assert not np.array_equal(oq["X"], pq["X"])


def test_8_the_chain_pid_laps_identify_game_laps(gpu, orc, golden_racing_game):
    """pid_laps -> identify() -> GameLaps(models=(fit.A, fit.B)) with the models never leaving the device.  The identified models are far
    from the shipped one: plumbing and agreement of the verdicts, not solver quality."""
    import torch
    from crx import montecarlo
    from utils import racing_env

    S = np.load(os.path.join(conftest.GOLDEN, "sysid.npz"))
    track = racing_env.ClosedTrack(S["track_spec"], track_width=1.0)
    n, T = 8, 600
    x0p = np.tile(S["short/x0"], (n, 1))
    vt = float(S["short/vt"]) * (1.0 + 0.05 * np.arange(n))
    laps = montecarlo.pid_laps(track.point_and_tangent, track.lap_length, x0p, x0p, T, vt=vt, noise_seed=3)
    fit = laps.identify(float(S["short/lamb"]))
    assert fit.A.is_cuda and fit.B.is_cuda and (fit.status.cpu().numpy() == 0).all()
    r, _ = _game(None, golden_racing_game, n, models=(fit.A, fit.B))
    assert r.track_models.A.data_ptr() == fit.A.data_ptr() and r.track_models.B.data_ptr() == fit.B.data_ptr()   # held, not copied
    assert r.plan_models.batch == n * (r.V + 1)
    r.step()   # (a CRX_ERR_* raises)
    ins, rg = _step0_regions(r)
    assert (r.m_ot.cpu().numpy() == 1).all() and np.isin(rg["status"], (0, 1, 2, 3, 5, 6)).all()
    mA, mB = fit.A.cpu().numpy(), fit.B.cpu().numpy()
    assert not np.array_equal(mA[0], mA[1])
    _regions_against_oracle("chain", orc, r, ins, rg, mA, mB, parity=False)
    assert ((rg["flag"] >= 0) & (rg["flag"] <= r.V)).all() and torch.isfinite(r.lm.xc).all()
