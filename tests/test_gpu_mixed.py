"""Mixed fields on the GPU: crx_mixed_prep_dev against the numpy model (tests/mixed_model.py) and, bit for bit, against crx_field_prep_dev
where they overlap; its independence of the launch's shape; crx_mixed_commit_dev against the model; crx.montecarlo.MixedRaces against the
FieldRaces it must reduce to, against each controller's own launch on the same inputs, and in a short noisy closed loop."""
import functools

import numpy as np
import pytest

import field_model as fm
import mixed_model as mm
import test_gpu_field as tf

pytestmark = pytest.mark.gpu

R_PREP = tf.R_PREP   # 37: a partial block for every C in 1 .. 7
N_PREP = 10
TRACKS = ("l_shape", "m_shape")
CARS = (1, 2, 4, 7)
N_ILQR = (0, 12, 50)
# the MPC_LTI comparison of test_each_car_gets_its_own_controllers_answer.  The suite had no bound for an NLP without obstacles solved in a launch
# WITH obstacle slots against the launch without them, so it is ten times the largest |U - U_zero_slot| measured there on an MI355X: 1.587e-07 at
# step 0 (the cars start 0.3 m/s below their targets), 3.789e-10 at step 7, both solves CRX_CONVERGED.  The margin covers two
# instantiations of one convex solve that stop at the same tolerance on different iterates
MPC_LTI_U_BOUND = 1.6e-6


@pytest.fixture(scope="module")
def gpu():
    import crx

    return crx.init(0)


def draw_policy(rng, R, C):
    """[R, C] codes: drawn per car, the last six cars of the launch one of each code, and (C >= 2) three constructed egos -- car 0 of race 0
    ILQR (it carries a whole lap: a non-zero il_lap_off), car 0 of race 3 ILQR (its last other car is the NaN car), car 0 of race 4 MPCCBF
    (race 4 repeats race 0's states: a kept car with lap offset L under the NLP family)."""
    pol = rng.integers(0, mm.N_POLICY, (R, C)).astype(np.int32)
    pol.reshape(-1)[-mm.N_POLICY:] = np.arange(mm.N_POLICY)
    if C >= 2:
        pol[0, 0], pol[3, 0], pol[4, 0] = mm.ILQR, mm.ILQR, mm.MPCCBF
    return pol


@functools.lru_cache(maxsize=None)
def draw(name, C, N, N_ilqr, seed, R=R_PREP):
    """(tab, L, x [R,C,6], dims [R,C,2], policy [R,C]): the states of test_gpu_field.draw -- races 0 .. 3 constructed, the rest drawn, all away
    from the thresholds of an N-step roll-out -- with race 4 a copy of race 0, and, as that draw does for its own horizon, every race drawn
    again (a constructed one in its free components) while the max(N, N_ilqr) + 1 steps rolled out HERE come within 1e-9 of a segment end or
    of the lap length, a window comparison within 1e-9 of its threshold, or the roll-out near the frame's singularity (|1 - curv ey| < 0.4:
    five seconds of zero input take one car in ten off the track, where field_model.predict says 1e-12 ends).  Asserts, on the CPU model
    alone, what the cases are there for."""
    tab, L, x, dims, _ = tf.draw(name, C, N, seed, R=R)
    x, dims = x.copy(), dims.copy()
    rng = np.random.default_rng(seed + 7919)
    race = lambda r: tf._fixed_race(rng, L, C, r) if r < tf.N_FIXED else tf._drawn_race(rng, L, C)   # noqa: E731
    pol = draw_policy(rng, R, C)
    for _ in range(200):
        x[4], dims[4] = x[0], dims[0]
        m = mm.prep(tab, L, x, pol, N, N_ilqr, car_dims=dims)
        with np.errstate(invalid="ignore"):
            bad = (m["edge"].min(axis=1) < 1e-9) | (m["gap"].min(axis=1) < 1e-9) | (m["cond"].min(axis=1) < 0.4)
        bad[4] = False                                                   # race 4 follows race 0
        if not bad.any():
            break
        for r in np.nonzero(bad)[0]:
            x[r] = race(r)
    else:
        raise AssertionError("the draw does not settle: %s" % np.nonzero(bad)[0])
    # the constructed states are still what test_gpu_field.draw built them to be
    f = fm.prep(tab, L, x, N, car_dims=dims)
    if C >= 2:
        assert f["n_obs"][0, 0] >= 1 and f["lap_off"][0, 0, 0] == L and f["n_obs"][2, 0] == C - 1
        assert f["n_obs"][1, 0] >= 1 and (np.diff(f["obs_s"][1, 0, 0]) < -0.5 * L).any()
    assert np.isnan(x[3, C - 1]).all() and np.isfinite(np.delete(x.reshape(-1, 6), 3 * C + C - 1, axis=0)).all()
    # what the policies are there for
    assert set(np.unique(pol)) == set(range(mm.N_POLICY))                # every policy occurs
    if C >= 2:
        cbf = pol == mm.MPCCBF
        kept = m["n_obs"][cbf].sum()
        assert 0 < kept < cbf.sum() * (C - 1)                            # MPCCBF cars keep some but not all opponents
        assert m["n_obs"][4, 0] >= 1 and m["lap_off"][4, 0, 0] == L and (m["n_obs"][~cbf] == 0).all() and not m["obs_s"][~cbf].any()
    if C >= 2 and N_ilqr > 0:
        for mode in (0, 1):
            mi = m if mode == 0 else mm.prep(tab, L, x, pol, N, N_ilqr, mode, car_dims=dims)
            il = pol == mm.ILQR
            assert (mi["il_lap_off"][il] != 0).any() and mi["il_lap_off"][0, 0, 0] == L        # an ILQR car with a non-zero lap offset
            assert mi["il_n_obs"][3, 0] == (C - 2 if mode else 0)                             # the NaN car is kept by nobody
            assert (mi["il_n_obs"][~il] == 0).all() and not mi["il_obs_s"][~il].any() and not np.isnan(mi["il_obs_s"]).any()
            n_fin = np.array([[len(mm.ilqr_slots(pol, mm.state_finite(x), e, r, mode)) for e in range(C)] for r in range(R)])
            assert np.array_equal(mi["il_n_obs"], n_fin) and mi["il_n_obs"][il].max() == (C - 1 if mode else 1)
    return tab, L, x, dims, pol


def _run(desc, tab, x, pol, dims=None, clear=True):
    """One crx_mixed_prep_dev launch; returns host arrays shaped as the model's."""
    import torch

    from crx import torch_api

    R, C = x.shape[:2]
    V, N1, NI1 = C - 1, desc.N + 1, desc.N_ilqr + 1
    dev = torch.device("cuda", 0)
    ws = torch_api.MixedWorkspace(desc, R, dev, dims=dims is not None, clear=clear)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)   # noqa: E731
    p = torch.as_tensor(np.ascontiguousarray(pol.reshape(-1)), dtype=torch.int32, device=dev)
    torch_api.mixed_prep_dev(desc, t(tab), t(x.reshape(R * C, 6)), p, ws, car_dims=None if dims is None else t(dims))
    torch.cuda.synchronize()
    out = dict(pred_s=ws.pred_s, pred_ey=ws.pred_ey, obs_s=ws.obs_s.reshape(R, C, V, N1), obs_ey=ws.obs_ey.reshape(R, C, V, N1),
               lap_off=ws.lap_off.reshape(R, C, V), n_obs=ws.n_obs.reshape(R, C), m_nlp=ws.m_nlp.reshape(R, C))
    if dims is not None:
        out["obs_dims"] = ws.obs_dims.reshape(R, C, V, 2)
    if desc.N_ilqr > 0:
        out.update(il_obs_s=ws.il_obs_s.reshape(R, C, V, NI1), il_obs_ey=ws.il_obs_ey.reshape(R, C, V, NI1),
                   il_lap_off=ws.il_lap_off.reshape(R, C, V), il_n_obs=ws.il_n_obs.reshape(R, C), m_ilqr=ws.m_ilqr.reshape(R, C))
    if clear:
        out["clear"] = ws.clear.reshape(R, C)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_prep(g, m, tag, use_dims, n_ilqr):
    ints = ("n_obs", "m_nlp") + (("il_n_obs", "m_ilqr") if n_ilqr else ())
    for k in ints:
        assert g[k].dtype == np.int32 and np.array_equal(g[k], m[k]), tag + (k,)
    for k in ("pred_s", "pred_ey", "obs_s", "obs_ey", "lap_off") + (("il_obs_s", "il_obs_ey", "il_lap_off") if n_ilqr else ()):
        np.testing.assert_allclose(g[k], m[k], rtol=0, atol=1e-12, equal_nan=True, err_msg=str(tag + (k,)))
    if use_dims:
        assert np.array_equal(g["obs_dims"], m["obs_dims"]), tag
    np.testing.assert_allclose(g["clear"], m["clear"], rtol=1e-12, atol=0, err_msg=str(tag))


@pytest.mark.parametrize("C", CARS)
def test_mixed_prep_matches_model(gpu, C):
    from crx import abi

    for name in TRACKS:
        for n_ilqr in N_ILQR:
            tab, L, x, dims, pol = draw(name, C, N_PREP, n_ilqr, 100 * C + n_ilqr)
            for mode in (0, 1):
                desc = abi.mixed_desc(N_PREP, n_ilqr, C, tab.shape[0], L, ilqr_obstacles=mode)
                for use_dims in (False, True):
                    tag = (name, C, n_ilqr, mode, use_dims)
                    d = dims if use_dims else None
                    m = mm.prep(tab, L, x, pol, N_PREP, n_ilqr, mode, car_dims=d)
                    g = _run(desc, tab, x, pol, d)
                    assert sorted(g) == sorted(k for k in m if k not in ("edge", "cond", "gap")), tag
                    _check_prep(g, m, tag, use_dims, n_ilqr)
                    # the NaN car poisons only its own roll-out
                    nan_row = np.isnan(g["pred_s"]).any(axis=-1)
                    assert nan_row.sum() == 1 and np.isnan(g["pred_s"][3, C - 1]).all() and np.isnan(g["pred_ey"][3, C - 1]).all(), tag
                    assert not np.isnan(g["obs_s"]).any() and not np.isnan(g["obs_ey"]).any(), tag
                    if n_ilqr:
                        assert not np.isnan(g["il_obs_s"]).any() and not np.isnan(g["il_obs_ey"]).any() and not np.isnan(g["il_lap_off"]).any(), tag


@pytest.mark.parametrize("C", CARS)
def test_mixed_prep_has_the_field_kernels_bits(gpu, C):
    """Columns 0 .. N of the roll-out, and every array of an MPCCBF car, are crx_field_prep_dev's on the same states, as bits."""
    from crx import abi

    for name in TRACKS:
        for n_ilqr in (0, 50):
            tab, L, x, dims, pol = draw(name, C, N_PREP, n_ilqr, 100 * C + n_ilqr)
            fdesc = abi.field_desc(N_PREP, C, tab.shape[0], L)
            mdesc = abi.mixed_desc(N_PREP, n_ilqr, C, tab.shape[0], L, ilqr_obstacles=1)
            for use_dims in (False, True):
                d = dims if use_dims else None
                f, g = tf._run(fdesc, tab, x, d), _run(mdesc, tab, x, pol, d)
                assert tf._same_bits(g["pred_s"][..., :N_PREP + 1], f["pred_s"]) and tf._same_bits(g["pred_ey"][..., :N_PREP + 1], f["pred_ey"])
                assert tf._same_bits(g["clear"], f["clear"])
                cbf = pol == mm.MPCCBF
                for k in ("obs_s", "obs_ey", "lap_off", "n_obs") + (("obs_dims",) if use_dims else ()):
                    assert tf._same_bits(g[k][cbf], f[k][cbf]), (name, C, n_ilqr, use_dims, k)


def test_mixed_prep_independence(gpu):
    """A race's outputs depend on nothing but the race: not on the other races, on how many there are, or on where it sits in the launch;
    and the host-pointer entry gives the bits of the device entry."""
    import crx
    from crx import abi

    C, n_ilqr, R = 4, 12, 150                                  # three blocks: 64 + 64 + 22 races
    tab, L, x, dims, pol = draw("l_shape", C, N_PREP, n_ilqr, 77, R=R)
    desc = abi.mixed_desc(N_PREP, n_ilqr, C, tab.shape[0], L, ilqr_obstacles=1)
    full = _run(desc, tab, x, pol, dims)
    _check_prep(full, mm.prep(tab, L, x, pol, N_PREP, n_ilqr, 1, car_dims=dims), ("independence",), True, n_ilqr)
    again = _run(desc, tab, x, pol, dims)
    for k in full:
        assert tf._same_bits(full[k], again[k]), k
    perm = np.random.default_rng(3).permutation(R)
    shuffled = _run(desc, tab, x[perm], pol[perm], dims[perm])
    for k in full:
        assert tf._same_bits(shuffled[k], full[k][perm]), k
    for pick in ([130], [2, 149, 70], list(range(60, 140))):   # other launch sizes, other blocks, other places in a block
        part = _run(desc, tab, x[pick], pol[pick], dims[pick])
        for k in full:
            assert tf._same_bits(part[k], full[k][pick]), (k, pick)
    host = crx.mixed_prep(desc, tab, x, pol, dims)
    assert sorted(host) == sorted(full)
    for k in full:
        assert tf._same_bits(np.asarray(host[k]), full[k]), k
    d0 = abi.mixed_desc(N_PREP, 0, C, tab.shape[0], L)         # no iLQR family, no dims, no clear: the arrays left out are not there
    plain_host, plain = gpu.mixed_prep(d0, tab, x, pol, None, clear=False), _run(d0, tab, x, pol, None, clear=False)
    assert sorted(plain_host) == sorted(plain) == ["lap_off", "m_nlp", "n_obs", "obs_ey", "obs_s", "pred_ey", "pred_s"]
    for k in plain:
        assert tf._same_bits(np.asarray(plain_host[k]), plain[k]), k


def _bits(a, b):
    """Equal as bits, up to the payload of a NaN: same shape and dtype, NaN where NaN, equal and equally signed elsewhere."""
    if not tf._same_bits(a, b):
        return False
    return a.dtype.kind != "f" or np.array_equal(np.signbit(a)[~np.isnan(a)], np.signbit(b)[~np.isnan(b)])


def test_mixed_commit_matches_model(gpu):
    import torch

    from crx import abi, torch_api

    Bn, N, Ni = 300, 10, 20
    rng = np.random.default_rng(18)
    pol = rng.integers(0, mm.N_POLICY, Bn).astype(np.int32)
    pol[:12] = np.repeat(np.arange(mm.N_POLICY), 2)                         # all six codes, with finite and (below) NaN states
    pol[12:17] = [-1, 6, 99, np.iinfo(np.int32).max, np.iinfo(np.int32).min]   # codes out of range
    x = rng.uniform(-1.0, 1.0, (Bn, 6))
    x[:, 0], x[:, 4] = rng.uniform(0.0, 2.0, Bn), rng.uniform(0.0, 40.0, Bn)
    x[1:12:2] = np.nan
    x[20, 3], x[21, 5], x[22, 0] = np.nan, np.inf, -np.inf
    vt, eyt = rng.uniform(0.3, 1.5, Bn), rng.uniform(-0.3, 0.3, Bn)
    K, xt = rng.standard_normal((Bn, 2, 6)), np.zeros((Bn, 6))
    xt[:, 0], xt[:, 5] = vt, eyt
    Un, Ui = rng.standard_normal((Bn, N, 2)), rng.standard_normal((Bn, Ni, 2))
    sn, si = rng.integers(0, 6, Bn).astype(np.int32), rng.integers(0, 6, Bn).astype(np.int32)
    assert set(np.unique(pol[17:])) == set(range(mm.N_POLICY)) and (sn != 0).any() and (si != 0).any()

    dev = torch.device("cuda", 0)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)   # noqa: E731
    dp, dx = t(pol), t(x)
    fams = dict(pid=(vt, eyt), lqr=(K, xt), nlp=(Un, sn), ilqr=(Ui, si))
    dfams = {k: tuple(t(a) for a in v) for k, v in fams.items()}

    def run(**kw):
        u = torch.full((Bn, 2), 7.0, dtype=torch.float64, device=dev)
        st = torch.full((Bn,), -7, dtype=torch.int32, device=dev)
        torch_api.mixed_commit_dev(dp, dx, u, st, **kw)
        torch.cuda.synchronize()
        return u.cpu().numpy(), st.cpu().numpy()

    u, st = run(**dfams)
    um, sm = mm.commit(pol, x, **fams)
    assert st.dtype == np.int32 and np.array_equal(st, sm) and _bits(u, um)
    skipped = ~np.isin(pol, [mm.PID, mm.LQR, mm.MPC_LTI, mm.MPCCBF, mm.ILQR])
    assert skipped[12:17].all() and (st[skipped] == abi.CRX_SKIPPED).all() and not u[skipped].any()
    assert (st[np.isin(pol, [mm.PID, mm.LQR])] == abi.CRX_CONVERGED).all()
    nlp, il = np.isin(pol, [mm.MPC_LTI, mm.MPCCBF]), pol == mm.ILQR
    assert np.array_equal(st[nlp], sn[nlp]) and np.array_equal(st[il], si[il])                    # a failed solve's status, its last iterate applied
    assert _bits(u[nlp], Un[nlp, 0]) and _bits(u[il], Ui[il, 0])
    # LQR against crx_lqr_step_dev: both are six-term sums within 6 eps sum|terms| of the exact value, one contracted, one not
    ul = torch.zeros((Bn, 2), dtype=torch.float64, device=dev)
    torch_api.lqr_step_dev(dfams["lqr"][0], dx, dfams["lqr"][1], ul)
    torch.cuda.synchronize()
    lq = (pol == mm.LQR) & np.isfinite(x).all(axis=1)
    assert lq.sum() >= 20
    bound = 16 * np.finfo(float).eps * np.abs(K * (x - xt)[:, None, :]).sum(axis=-1)
    assert (np.abs(u - ul.cpu().numpy())[lq] <= bound[lq]).all()
    # a family passed as NULL: its cars get zero and CRX_SKIPPED, every other car is unchanged
    codes = dict(pid=[mm.PID], lqr=[mm.LQR], nlp=[mm.MPC_LTI, mm.MPCCBF], ilqr=[mm.ILQR])
    for gone in fams:
        u2, st2 = run(**{k: v for k, v in dfams.items() if k != gone})
        um2, sm2 = mm.commit(pol, x, **{k: v for k, v in fams.items() if k != gone})
        off = np.isin(pol, codes[gone])
        assert off.any() and not u2[off].any() and (st2[off] == abi.CRX_SKIPPED).all(), gone
        assert _bits(u2[~off], u[~off]) and np.array_equal(st2[~off], st[~off]) and _bits(u2, um2) and np.array_equal(st2, sm2), gone
    u3, st3 = run()
    assert not u3.any() and (st3 == abi.CRX_SKIPPED).all()


# ---- the closed loop -------------------------------------------------------------------------------------------------------------------
def _field(R, C, seed):
    """R races of C cars on l_shape, 1.5 m apart from a drawn point, on four lines; target speeds that make them meet."""
    track = tf._track("l_shape", 1.0)
    tab, L = track.point_and_tangent, track.lap_length
    rng = np.random.default_rng(seed)
    x0 = np.zeros((R, C, 6))
    x0[..., 0] = 0.3
    x0[..., 4] = (rng.uniform(0.0, L, (R, 1)) + 1.5 * np.arange(C)[None, :]) % L
    x0[..., 5] = rng.choice([-0.3, -0.1, 0.1, 0.3], (R, C))
    g0 = tf._globals(track, x0.reshape(-1, 6))
    vt = np.sort(rng.uniform(0.5, 1.0, (R, C)), axis=1)[:, ::-1].copy()      # the car behind is the faster one
    return track, tab, L, x0, g0, vt


def _family(AB, n, s, seed):
    g = np.random.default_rng(seed)
    return (np.array([AB[0] * (1 + s * g.standard_normal((6, 6))) for _ in range(n)]),
            np.array([AB[1] * (1 + s * g.standard_normal((6, 2))) for _ in range(n)]))


@pytest.mark.parametrize("how", ["car_dims", "models"])
def test_all_mpccbf_retraces_field_races(gpu, AB, how):
    """MixedRaces with every car MPCCBF is FieldRaces, bit for bit, over 20 noisy steps."""
    from crx import montecarlo

    R, C, N, steps = 9, 4, 10, 20
    track, tab, L, x0, g0, vt = _field(R, C, 5)
    kw = dict(vt=vt, N=N, noise_seed=11)
    if how == "car_dims":
        rng = np.random.default_rng(6)
        kw["car_dims"] = np.stack([rng.uniform(0.3, 0.5, (R, C)), rng.uniform(0.15, 0.25, (R, C))], axis=-1)
    else:
        kw["models"] = _family(AB, R * C, 1e-2, 9)
    f = montecarlo.FieldRaces(tab, L, track.width, AB[0], AB[1], x0, g0, C, **kw)
    m = montecarlo.MixedRaces(tab, L, track.width, AB[0], AB[1], x0, g0, np.full((R, C), "mpccbf"), **kw)
    assert m.iws is None and m.K is None and m.vt is None and m.mdesc.N_ilqr == 0
    for k in range(steps):
        f.step(); m.step()
        for name, a, b in (("xc", f.xc, m.xc), ("u", f.u, m.u), ("status", f.ws.status, m.status), ("min_clear", f.min_clear, m.min_clear)):
            assert _bits(a.cpu().numpy(), b.cpu().numpy()), (how, k, name)
    assert np.isfinite(m.xc.cpu().numpy()).all() and (m.mws.n_obs.cpu().numpy() > 0).any()


POLICY_ROW = ("mpccbf", "ilqr", "pid", "lqr")


def _mixed(AB, seed=21, races=None, noise=None, **kw):
    """The R = 6, C = 4 field of tests 6 and 7: five races of (MPCCBF, ILQR, PID, LQR), one with MPC_LTI and NONE in it."""
    from crx import montecarlo

    R, C = 6, 4
    track, tab, L, x0, g0, vt = _field(R, C, seed)
    pol = np.array([POLICY_ROW] * R, dtype="U8")
    pol[2] = ("mpc_lti", "none", "mpccbf", "ilqr")
    pick = slice(None) if races is None else races
    r = montecarlo.MixedRaces(tab, L, track.width, AB[0], AB[1], x0[pick], g0.reshape(R, C, 6)[pick], pol[pick], vt=vt[pick], N=10, ilqr_N=20,
                              ilqr_max_iter=20, noise_seed=noise, **kw)
    return r, pol[pick]


def test_each_car_gets_its_own_controllers_answer(gpu, AB):
    """At steps 0 and 7 the input a car applied is stage 0 of ITS controller's plan on the step's prep outputs: the ILQR cars re-solved as a
    compacted batch through ilqr_solve_dev, the NLP cars through cbf_solve_dev (batch independence of both kernels is pinned elsewhere);
    cars outside a mask are skipped and their workspace rows untouched; an MPC_LTI car's plan is the zero-slot launch's that SeedLaps uses."""
    import torch

    from crx import abi, torch_api

    r, pol = _mixed(AB)
    codes = abi.policy_codes(pol).reshape(-1)
    nlp, il = np.isin(codes, [mm.MPC_LTI, mm.MPCCBF]), codes == mm.ILQR
    lti = codes == mm.MPC_LTI
    dev = r.device
    ix = lambda mask: torch.as_tensor(np.nonzero(mask)[0], device=dev)   # noqa: E731
    worst = 0.0
    for k in range(8):
        if k in (0, 7):                                                  # rows no launch of this step may touch
            for ws, mask in ((r.ws, nlp), (r.iws, il)):
                for a in (ws.X, ws.U, ws.cost):
                    a[ix(~mask)] = -77.0
        r.step()
        if k not in (0, 7):
            continue
        x0, m = r.xc_next, r.mws                                         # the state the step started from, and its prep outputs
        u, st = r.u.cpu().numpy(), r.status.cpu().numpy()
        sel = lambda a, mask: a[ix(mask)].contiguous()   # noqa: E731
        wi = torch_api.ilqr_solve_dev(r.idesc, sel(x0, il), sel(r.xt, il), sel(m.il_obs_s, il), sel(m.il_obs_ey, il), sel(m.il_lap_off, il),
                                      sel(m.il_n_obs, il))
        wn = torch_api.cbf_solve_dev(r.desc, sel(x0, nlp), sel(r.xt, nlp), sel(m.obs_s, nlp), sel(m.obs_ey, nlp), sel(m.lap_off, nlp), sel(m.n_obs, nlp))
        torch.cuda.synchronize()
        assert _bits(wi.U[:, 0].cpu().numpy(), u[il]) and np.array_equal(wi.status.cpu().numpy(), st[il]), k
        assert _bits(wn.U[:, 0].cpu().numpy(), u[nlp]) and np.array_equal(wn.status.cpu().numpy(), st[nlp]), k
        assert (m.il_n_obs.cpu().numpy()[il] == 1).all() and (m.n_obs.cpu().numpy()[lti] == 0).all()
        # outside a mask: CRX_SKIPPED and untouched rows
        for ws, mask in ((r.ws, nlp), (r.iws, il)):
            assert (ws.status.cpu().numpy()[~mask] == abi.CRX_SKIPPED).all() and (ws.status.cpu().numpy()[mask] != abi.CRX_SKIPPED).all()
            for a in (ws.X, ws.U, ws.cost):
                assert (a.cpu().numpy()[~mask] == -77.0).all()
        # pid, lqr, none: the model's law on the same state
        um, sm = mm.commit(codes, x0.cpu().numpy(), pid=(r.vt.cpu().numpy(), r.eyt.cpu().numpy()), lqr=(r.K.cpu().numpy(), r.xt.cpu().numpy()))
        rest = ~(nlp | il)
        assert _bits(u[rest], um[rest]) and np.array_equal(st[rest], sm[rest]) and (st[codes == mm.NONE] == abi.CRX_SKIPPED).all()
        # the MPC_LTI car against the launch without obstacle slots (the budgets of the launch it ran in: cbf_desc would give the one-slot class others)
        d0 = abi.cbf_desc(r.N, 0, AB[0], AB[1], alpha=0.8, margin=0.2, ey_max=r.track_width, opts=abi.default_opts(**abi.cbf_class_budgets(r.N, r.n_cars - 1)))
        n = int(lti.sum())
        none = (torch.zeros((n, 0, r.N + 1), dtype=torch.float64, device=dev), torch.zeros((n, 0, r.N + 1), dtype=torch.float64, device=dev),
                torch.zeros((n, 0), dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
        w0 = torch_api.cbf_solve_dev(d0, sel(x0, lti), sel(r.xt, lti), *none)
        torch.cuda.synchronize()
        assert np.array_equal(w0.status.cpu().numpy(), r.ws.status.cpu().numpy()[lti]), k
        diff = float(np.abs(w0.U.cpu().numpy() - r.ws.U.cpu().numpy()[lti]).max())
        worst = max(worst, diff)
        print("mixed: step %d, MPC_LTI plan against the zero-slot launch: max |dU| = %.3e (status %s)" % (k, diff, w0.status.cpu().numpy()))
    assert worst <= MPC_LTI_U_BOUND, worst


class _SliceNoise:
    """The rows `rows` of the draws a loop of `total` cars makes from `seed`: what a race run alone must see to be the race of the big run."""

    def __init__(self, seed, device, total, rows):
        from crx import montecarlo

        self.inner, self.total, self.rows = montecarlo._Noise(seed, device), total, rows

    def draw(self, batch):
        return self.inner.draw(self.total)[self.rows].contiguous()


def test_mixed_closed_loop(gpu, AB):
    """25 noisy steps of the mixed field: finite, RaceStats attaches, passes made = passes suffered per race, and a race of the launch is the
    race run alone, bit for bit."""
    import torch

    from crx import montecarlo

    R, C, steps = 6, 4, 25
    r, pol = _mixed(AB, noise=13)
    group = torch.arange(R, dtype=torch.int32).repeat_interleave(C)
    stats = montecarlo.RaceStats(r, group=group, n_groups=R)
    lone = {}
    for race in (2, 5):
        lone[race], _ = _mixed(AB, races=[race])
        lone[race].noise = _SliceNoise(13, r.device, R * C, slice(race * C, (race + 1) * C))
    stats.update()
    for k in range(steps):
        stats.step()
        for race, q in lone.items():
            q.step()
            rows = slice(race * C, (race + 1) * C)
            for name, a, b in (("xc", r.xc, q.xc), ("u", r.u, q.u), ("status", r.status, q.status), ("min_clear", r.min_clear, q.min_clear)):
                assert _bits(a[rows].cpu().numpy(), b.cpu().numpy()), (race, k, name)
    assert np.isfinite(r.xc.cpu().numpy()).all() and np.isfinite(r.u.cpu().numpy()).all() and np.isfinite(r.min_clear.cpu().numpy()).all()
    recs = stats.summary()
    assert len(recs) == R and all(rec["cars"] == C and rec["n_samples"] == C * (steps + 1) and rec["nonfinite"] == 0 for rec in recs)
    assert all(rec["passes"] == rec["passed"] for rec in recs), [(rec["passes"], rec["passed"]) for rec in recs]
    per = stats.per_car()
    np.testing.assert_allclose(per["min_clear"], np.minimum(r.min_clear.cpu().numpy(), montecarlo_clear_last(r)), rtol=1e-12, atol=0)
    print("mixed closed loop: passes per race %s, min_clear %.3f, contacts %d" % ([rec["passes"] for rec in recs], recs and min(rec["min_clear"] for rec in recs),
                                                                               sum(rec["contact"] for rec in recs)))


def montecarlo_clear_last(r):
    """`clear` of the states a loop holds now (the sample RaceStats took after the last step, which no prep launch has seen yet)."""
    return fm.clear(r.xc.cpu().numpy().reshape(r.n_races, r.n_cars, 6), r.lap_length).reshape(-1)
