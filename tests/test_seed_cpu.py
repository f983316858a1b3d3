"""Seed laps without a GPU and without the library (include/crx.h "Seed laps", S1-S6; crx.montecarlo.SeedLaps).

(a) tests/seed_model.py, the NumPy model the kernels are held to, against the reference's own recording of its PID lap and its MPC-LTI lap
(tests/golden/racing_game.npz): driven with the recorded states it reproduces the recorded PID inputs, both lap logs, the phase changes at
steps 294 and 554, and -- through the oracle's add-trajectory -- the reference's safe set, all exactly.
(b) The launch sequence of SeedLaps.step() under a recorder that stands in for crx.torch_api, in the manner of
tests/test_montecarlo_sequence_cpu.py.
(c) montecarlo._dev with tensors."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import seed_model
from crx import abi, montecarlo, torch_api


def _oracle_addtraj(lib, d, crossed, log_x, log_u, n_log, ss, us, qf, time_ss, it, step, x):
    status = np.zeros(len(crossed), dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = lib.crx_oracle_lmpc_addtraj(C.byref(d), C.c_int(len(crossed)), p(crossed), p(log_x), p(log_u), p(n_log), p(ss), p(us), p(qf),
                                     p(time_ss), p(it), p(step), p(x), p(status))
    assert rc == 0
    return status


def test_model_against_the_reference_recording(golden_racing_game):
    import oracle
    oracle.load()
    lib = C.CDLL(oracle._LIB)
    g = golden_racing_game
    Bn, L = 2, float(g["lap_length"])                       # two copies of the reference's car
    P, NL = g["ss/ss0"].shape[0], g["ss/ss0"].shape[2]
    laps_x, laps_g, laps_u = [g["lap%d/xcurv" % k] for k in (0, 1)], [g["lap%d/xglob" % k] for k in (0, 1)], [g["lap%d/u" % k] for k in (0, 1)]
    T0, T1 = len(laps_u[0]), len(laps_u[1])
    assert (T0, T1) == (294, 260)
    off = np.array([0, 0, 0, 0, L, 0])
    np.testing.assert_array_equal(laps_x[1][0], laps_x[0][-1] - off)
    tile = lambda a: np.tile(np.asarray(a)[None], (Bn,) + (1,) * np.ndim(a))   # noqa: E731
    st = seed_model.State(tile(laps_x[0][0]), P)
    vt, eyt = np.full(Bn, 0.7), np.zeros(Bn)
    d = abi.lmpcprep_desc(12, P, NL, 9, float(g["timestep"]), L)
    ss, us, qf = np.full((Bn, NL, P, 6), 10000.0), np.full((Bn, NL, P, 2), 10000.0), np.zeros((Bn, NL, P))
    time_ss, it, step = np.full((Bn, NL), 10000, dtype=np.int32), np.zeros(Bn, dtype=np.int32), np.zeros(Bn, dtype=np.int32)
    xc, xg = tile(laps_x[0][0]), tile(laps_g[0][0])
    k_total, phases, masks = 0, [], []
    for lap in (0, 1):
        T = len(laps_u[lap])
        for k in range(T):
            # the solver's plan of this step, as the recording has its first stage; lap 0 must not read it
            U_mpc = np.full((Bn, 10, 2), np.nan) if lap == 0 else tile(np.vstack([laps_u[1][k]] + [np.zeros(2)] * 9))
            status = np.full(Bn, 4 if lap == 0 else 0, dtype=np.int32)          # CRX_SKIPPED under the mask, converged in the MPC-LTI lap
            np.testing.assert_array_equal(st.m_mpc, lap)
            seed_model.commit(st.phase, vt, eyt, xc, U_mpc, status, st.seed_status, st.u)
            np.testing.assert_array_equal(st.u, tile(laps_u[lap][k]))           # S1: the recorded PID inputs, bit for bit; S2
            # the plant, from the recording: the state after the step, wrapped at the line (update_memory)
            xc_prev, xg_prev = xc, xg
            cross = k + 1 == T
            xc, xg = tile(laps_x[lap][k + 1] - (off if cross else 0.0)), tile(laps_g[lap][k + 1])
            st.laps += int(cross)
            seed_model.log(L, xc_prev, xg_prev, xc, xg, st.u, st.laps, st.laps_prev, st.log_x, st.log_u, st.n_log, st.crossed, st.phase,
                           st.seed_status, st.m_mpc)
            k_total += 1
            phases.append(st.phase.copy()); masks.append(st.m_mpc.copy())
            np.testing.assert_array_equal(st.crossed, int(cross))
            if cross:                                                           # the lap's log is the recorded lap
                for b in range(Bn):
                    np.testing.assert_array_equal(st.log_x[b, :T + 1], laps_x[lap])
                    np.testing.assert_array_equal(st.log_u[b, :T], laps_u[lap])
                    assert st.n_log[b] == T + 1
            s = _oracle_addtraj(lib, d, st.crossed, st.log_x, st.log_u, st.n_log, ss, us, qf, time_ss, it, step, xc)
            assert (s == 0).all()
    phases, masks = np.array(phases), np.array(masks)
    assert k_total == T0 + T1 == 554
    assert (phases[:T0 - 1] == 0).all() and (phases[T0 - 1:T0 + T1 - 1] == 1).all() and (phases[T0 + T1 - 1] == 2).all()   # 0 -> 1 at step 294, 1 -> 2 at 554
    np.testing.assert_array_equal(masks, (phases == 1).astype(np.int32))
    assert (st.seed_status == 0).all() and (it == 2).all() and (st.n_log == 1).all()
    # the safe set the reference built from the same two laps
    ref_ss = np.ascontiguousarray(g["ss/ss0"].transpose(2, 0, 1)); ref_u = np.ascontiguousarray(g["ss/u0"].transpose(2, 0, 1))
    ref_q = np.ascontiguousarray(g["ss/Qfun0"].T)
    for b in range(Bn):
        np.testing.assert_array_equal(ss[b], ref_ss)
        np.testing.assert_array_equal(us[b], ref_u)
        np.testing.assert_array_equal(qf[b], ref_q)
        np.testing.assert_array_equal(time_ss[b], g["ss/time_ss"])
    np.testing.assert_array_equal(xc[0], g["lmpc/x"][0])                        # the hand-over state is where the recorded learning-MPC lap starts
    # a third, frozen stretch (S4): the plant steps the car from the same state every time and its output "crosses"; nothing of the car moves
    keep = {k: v.copy() for k, v in vars(st).items()}
    hand_c, hand_g = xc.copy(), xg.copy()
    for k in range(3):
        seed_model.commit(st.phase, vt, eyt, xc, np.full((Bn, 10, 2), np.nan), np.full(Bn, 4, dtype=np.int32), st.seed_status, st.u)
        np.testing.assert_array_equal(st.u, 0.0)                                # S3
        out_c, out_g = xc + 0.01, xg + 0.02
        st.laps += 1
        seed_model.log(L, xc, xg, out_c, out_g, st.u, st.laps, st.laps_prev, st.log_x, st.log_u, st.n_log, st.crossed, st.phase, st.seed_status,
                       st.m_mpc)
        xc, xg = out_c, out_g
        np.testing.assert_array_equal(xc, hand_c); np.testing.assert_array_equal(xg, hand_g)
        for name, v in keep.items():
            if name not in ("u", "crossed"):                                    # (the commit's output; S4 clears the flag)
                np.testing.assert_array_equal(getattr(st, name), v, err_msg=name)
        np.testing.assert_array_equal(st.crossed, 0)


def test_model_log_full_and_failed_solve():
    """S6's other branch and S2's flag, on two cars with three log rows: car 0 never reaches the line, car 1 crosses with its last row."""
    st = seed_model.State(np.zeros((2, 6)), 3)
    st.phase[:] = 1
    xc, xg = np.ones((2, 6)), np.ones((2, 6))
    U = np.arange(8.0).reshape(2, 2, 2)
    seed_model.commit(st.phase, np.ones(2), np.zeros(2), xc, U, np.array([1, 0], dtype=np.int32), st.seed_status, st.u)
    np.testing.assert_array_equal(st.u, U[:, 0]); np.testing.assert_array_equal(st.seed_status, [1, 0])
    for k in range(2):
        if k == 1:
            st.laps[1] += 1
        new_c = xc + 1.0
        seed_model.log(20.0, xc, xg, new_c, xg + 1.0, st.u, st.laps, st.laps_prev, st.log_x, st.log_u, st.n_log, st.crossed, st.phase,
                       st.seed_status, st.m_mpc)
        xc = new_c
    np.testing.assert_array_equal(st.phase, [3, 2]); np.testing.assert_array_equal(st.seed_status, [1 | 2, 0])
    np.testing.assert_array_equal(st.m_mpc, [0, 0]); np.testing.assert_array_equal(st.n_log, [3, 3])
    assert st.log_x[1, 2, 4] == 3.0 + 20.0 and st.log_x[0, 2, 4] == 3.0       # the crossing state is logged with s unwrapped


# ---- the launch sequence ---------------------------------------------------------------------------------------------------------------------
BN = 3
TAB, LAP, WIDTH = np.zeros((5, 6)), 20.0, 1.0


class _Models:
    def __init__(self, rec, desc, A, B):
        self.A, self.B = A, B
        rec.calls.append(("crx_cbf_models_reach_dev", dict(desc=desc, A=A, B=B)))


class Recorder:
    """Stands in for crx.torch_api: classes and constants are the real ones, every `*_dev` wrapper and longest_first is recorded as
    (name, arguments by parameter name) and launches nothing."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        real = getattr(torch_api, name)
        if name == "CbfModels":
            return lambda desc, A, B: _Models(self, desc, A, B)
        if not (name.endswith("_dev") or name == "longest_first"):
            return real
        sig = inspect.signature(real)

        def record(*a, **kw):
            args = sig.bind(*a, **kw)
            args.apply_defaults()
            args = dict(args.arguments)
            self.calls.append((name, args))
            if name == "longest_first":
                return torch.zeros(args["iters"].shape[0], dtype=torch.int32)
            return args.get("ws")

        return record

    def take(self):
        calls, self.calls = self.calls, []
        return [n for n, _ in calls], dict(calls)


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(montecarlo, "torch_api", r)
    return r


SEED_STEP = ["cbf_solve_dev", "seed_commit_dev", "plant_step_wrap_dev", "seed_log_dev", "lmpc_addtraj_dev"]


@pytest.mark.parametrize("models", [False, True])
def test_seed_laps_sequence(rec, AB, models):
    z = np.zeros((BN, 6))
    kw = dict(models=(np.tile(AB[0], (BN, 1, 1)), np.tile(AB[1], (BN, 1, 1)))) if models else {}
    r = montecarlo.SeedLaps(TAB, LAP, WIDTH, AB[0], AB[1], z, z, vt=[0.5, 0.6, 0.7], n_points=30, device="cpu", **kw)
    assert rec.take()[0] == (["crx_cbf_models_reach_dev"] if models else [])
    # control.mpc_lti's problem: no obstacle slot, MPCTrackingParam's weights, the track's width; the safe set as LMPCRacingGame.__init__ leaves it
    assert r.desc.n_obs_max == 0 and r.desc.N == 10 and list(r.desc.Q) == [10.0, 0.0, 0.0, 4.0, 0.0, 40.0] and list(r.desc.R) == [0.1, 0.1]
    assert r.desc.ey_max == WIDTH
    assert tuple(r.ss.shape) == (BN, 4, 30, 6) and (r.ss == 10000.0).all() and (r.us == 10000.0).all() and (r.qf == 0.0).all()
    assert (r.time_ss == 10000).all() and (r.it == 0).all() and (r.phase == 0).all() and (r.m_mpc == 0).all() and (r.n_log == 1).all()
    assert torch.equal(r.xt[:, 0], torch.tensor([0.5, 0.6, 0.7], dtype=torch.float64)) and torch.equal(r.vt, r.xt[:, 0])
    for k in range(2):
        xg, xc, xg_next, xc_next = r.xg, r.xc, r.xg_next, r.xc_next
        r.step()
        names, args = rec.take()
        assert names == SEED_STEP
        solve, commit, plant, log, traj = (args[n] for n in SEED_STEP)
        assert solve["active"] is r.m_mpc and solve["x0"] is xc and solve["xt"] is r.xt and solve["ws"] is r.ws and solve["order"] is None
        assert solve["models"] is r.models and (r.models is not None) == models and solve["desc"] is r.desc
        assert commit["x"] is xc and commit["U_mpc"] is r.ws.U and commit["mpc_status"] is r.ws.status and commit["u"] is r.u
        assert commit["phase"] is r.phase and commit["seed_status"] is r.seed_status and commit["vt"] is r.vt and commit["eyt"] is r.eyt
        # the plant reads and writes the bound pairs and they swap
        assert plant["desc"] is r.plant and plant["track"] is r.tab and plant["laps"] is r.laps and plant["u"] is r.u and plant["u_stride"] == 2
        assert plant["xglob"] is xg and plant["xcurv"] is xc and plant["xglob_next"] is xg_next and plant["xcurv_next"] is xc_next
        assert r.xg is xg_next and r.xc is xc_next and r.xg_next is xg and r.xc_next is xc
        # the log is given the pre-swap pair as *_prev and what the plant wrote as the pair it may overwrite
        assert log["xcurv_prev"] is xc and log["xglob_prev"] is xg and log["xcurv"] is xc_next and log["xglob"] is xg_next
        assert log["u"] is r.u and log["phase"] is r.phase and log["m_mpc"] is r.m_mpc and log["crossed"] is r.crossed and log["laps"] is r.laps
        assert traj["crossed"] is r.crossed and traj["x"] is r.xc and traj["ss_xcurv"] is r.ss and traj["it"] is r.it and traj["log_x"] is r.log_x
        assert r.k == k + 1
    r.dispatch = "longest_first"
    r.step()
    names, args = rec.take()
    assert names == ["longest_first"] + SEED_STEP
    assert args["longest_first"]["iters"] is r.ws.iters and args["longest_first"]["active"] is r.m_mpc and args["cbf_solve_dev"]["order"] is not None


def test_seed_laps_hand_over(rec, AB):
    """lmpc_inputs(): the loop's own tensors and two slices of them; LmpcLaps and GameLaps take them as they are and own copies; a
    RaceStats reads the loop through the inherited stats_inputs()."""
    z = np.zeros((BN, 6))
    r = montecarlo.SeedLaps(TAB, LAP, WIDTH, AB[0], AB[1], z, z, n_points=30, device="cpu")
    r.ss.copy_(torch.arange(r.ss.numel(), dtype=torch.float64).reshape(r.ss.shape))
    r.us.copy_(torch.arange(r.us.numel(), dtype=torch.float64).reshape(r.us.shape))
    r.time_ss[:, :2] = 20; r.it[:] = 2
    inp = r.lmpc_inputs()
    assert list(inp) == ["ss_xcurv", "u_ss", "qfun", "time_ss", "it", "xcurv0", "xglob0", "lin_points", "lin_input"]
    assert inp["ss_xcurv"] is r.ss and inp["xcurv0"] is r.xc and inp["xglob0"] is r.xg and inp["it"] is r.it
    assert torch.equal(inp["lin_points"], r.ss[:, 0, 1:14]) and torch.equal(inp["lin_input"], r.us[:, 0, 1:13])
    lm = montecarlo.LmpcLaps(TAB, LAP, WIDTH, **inp, device="cpu")
    assert lm.ss is not r.ss and lm.ss.data_ptr() != r.ss.data_ptr() and torch.equal(lm.ss, r.ss) and lm.xc.data_ptr() != r.xc.data_ptr()
    assert lm.time_ss.dtype == torch.int32 and torch.equal(lm.time_ss, r.time_ss) and lm.lin_points.is_contiguous()
    assert tuple(lm.lin_points.shape) == (BN, 13, 6) and tuple(lm.lin_input.shape) == (BN, 12, 2)
    cars = np.full((BN, 2), 3.0), np.full((BN, 2), 0.2), np.zeros((BN, 2))
    g = montecarlo.GameLaps(TAB, LAP, WIDTH, AB[0], AB[1], np.zeros((7, 6)), *(inp[k] for k in inp), *cars, device="cpu")
    assert torch.equal(g.lm.us, r.us) and g.lm.us.data_ptr() != r.us.data_ptr()
    s = r.stats_inputs()
    assert s["xcurv"] is r.xc and s["laps"] is r.laps and s["track_width"] == WIDTH and s["xt"] is r.xt


def test_dev_with_tensors():
    dev = torch.device("cpu")
    t = torch.arange(12, dtype=torch.float64).reshape(2, 6)
    same = montecarlo._dev(t, dev)
    assert same.data_ptr() == t.data_ptr()                                    # nothing to do: the caller's tensor
    own = montecarlo._dev(t, dev, clone=True)
    assert own.data_ptr() != t.data_ptr() and torch.equal(own, t)
    own[0, 0] = -1.0
    assert t[0, 0] == 0.0
    i = montecarlo._dev(torch.tensor([3, 4], dtype=torch.int64), dev, torch.int32, clone=True)
    assert i.dtype == torch.int32 and i.tolist() == [3, 4]
    sl = montecarlo._dev(torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)[:, 1:], dev, clone=True)
    assert sl.is_contiguous() and tuple(sl.shape) == (2, 2, 4)
    # host arrays take the path they took: float64, contiguous; without clone the CPU tensor shares the caller's array, with clone it does not
    a = np.arange(12.0).reshape(2, 6)
    shared, copied = montecarlo._dev(a, dev), montecarlo._dev(a, dev, clone=True)
    a[0, 0] = 7.0
    assert shared[0, 0] == 7.0 and copied[0, 0] == 0.0 and shared.dtype == torch.float64
    assert montecarlo._dev(np.arange(6).reshape(2, 3).T, dev).is_contiguous()
    assert montecarlo._dev([1, 2], dev, torch.int32).dtype == torch.int32


def test_abi_declares_the_seed_entries():
    """The signatures torch_api calls through: the header's argument lists (ints and the lap length by value, then pointers and the stream)."""
    import os
    import re

    import conftest
    src = open(os.path.join(conftest.ROOT, "include", "crx.h")).read()
    for name, argtypes in abi.SEED_ARGTYPES.items():
        decl = re.search(r"int crx_%s\((.*?)\);" % name, src, re.S).group(1)
        params = [p.strip() for p in decl.split(",")]
        assert len(params) == len(argtypes), name
        for p, t in zip(params, argtypes):
            want = C.c_void_p if "*" in p else (C.c_double if p.startswith("double") else C.c_int)
            assert t is want, (name, p)
