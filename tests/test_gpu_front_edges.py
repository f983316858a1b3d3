"""The kernels between the raw race state and a solver launch -- crx_scene_kernel, crx_prep_kernel, crx_select_kernel,
crx_trackprep_kernel, crx_cbfprep_kernel, crx_cbfprep_laps_kernel, crx_game_traffic_kernel -- on the edges of their comparisons.
GPU box only.

Every case of tests/golden/front_edges.npz (the reference's own decisions with the deciding quantity exactly on its edge and one
np.nextafter to either side; tests/golden/tools/make_front_edges.py) goes through the device entries and must give the recorded
answer and what tests/front_model.py gives: decisions, integers and copies bit for bit, Bezier polylines to 1e-14, per-stage
targets to 1e-13 (tests/front_edges_cases.py).  tests/test_front_edges_cpu.py holds the model, the host mirror and the oracle to
the same file.  Two more launches per kernel for what edge data alone does not show:
    locality     the scenes of the launch permuted: every scene keeps its bits
    batch edges  (the one-thread-per-race kernels, blocks of 256) the set tiled to 257 races and a single race, every output one race
                 longer than the batch and pre-filled: the slot past the batch keeps the fill, the others equal the untiled answers
"""
import numpy as np
import pytest

import front_edges_cases as fc

pytestmark = pytest.mark.gpu

FILL_F, FILL_I = -7777.0, -77


@pytest.fixture(scope="module")
def gpu():
    import crx

    return crx.init()


@pytest.fixture(scope="module")
def Z():
    return fc.load()


def _perm(n, seed):
    return np.random.default_rng(seed).permutation(n)


def _same(a, b, keys, idx, what):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k][idx], err_msg="%s: %s" % (what, k))


# ---- one wave per scenario ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,VA,V", [(10, 6, 3), (12, 8, 6)])
def test_scene(gpu, Z, N, VA, V):
    from crx import abi

    b = fc.scene_batch(Z, N, VA, V)
    d = abi.scene_desc(N, VA, V, b["L"], veh_length=b["length"])
    run = lambda i: gpu.planner_scene(d, b["ego"][i], b["n_all"][i], b["veh"][i], b["pred_s"][i], b["pred_ey"][i])   # noqa: E731
    res = run(slice(None))
    fc.check_scene(res, b)
    p = _perm(len(b["names"]), 1)
    _same(run(p), res, fc.SCENE_KEYS, p, "permuted launch")


@pytest.mark.parametrize("N,V", [(10, 3), (12, 6)])
def test_prep(gpu, Z, N, V):
    from crx import abi

    b = fc.prep_batch(Z, N, V)
    S, R = len(b["names"]), V + 1
    d = abi.prep_desc(N, V, len(b["opt_s"]), b["track_width"], b["L"], veh_length=b["length"], veh_width=b["width"])

    def run(i):
        r = gpu.planner_prep(d, b["x_wrapped"][i], b["x_raw"][i], b["n_veh"][i], b["veh_info"][i], b["max_dv"][i], b["obs_s"][i], b["obs_ey"][i],
                             b["opt_s"], b["opt_ey"])
        return {k: v.reshape((S, R) + v.shape[1:]) for k, v in r.items()}

    res = run(slice(None))
    fc.check_prep(res, b)
    p = _perm(S, 2)
    _same(run(p), res, ("bez_s", "bez_ey", "ey_lb", "ey_ub", "x0"), p, "permuted launch")


@pytest.mark.parametrize("N,V", [(10, 3), (12, 6)])
def test_select(gpu, Z, N, V):
    from crx import abi

    b = fc.select_batch(Z, N, V)
    d = abi.select_desc(N, V, b["L"], veh_length=b["length"], veh_width=b["width"])
    run = lambda i: gpu.select(d, b["n_veh"][i], b["X"][i], b["obs_s"][i], b["obs_ey"][i], b["old_flag"][i])   # noqa: E731
    res = run(slice(None))
    fc.check_select(res, b)
    p = _perm(len(b["names"]), 3)
    _same(run(p), res, fc.SELECT_KEYS, p, "permuted launch")


# ---- one thread per race: outputs one race longer than the batch, pre-filled ------------------------------------------------------
class Guarded:
    """Output tensors of a launch of n races, allocated for n + 1 and filled; `views` are the first n, `check` the last."""

    def __init__(self, n, shapes):
        import torch

        dev = torch.device("cuda", 0)
        self.n, self.full = n, {}
        for k, (shape, dt) in shapes.items():
            fill = FILL_I if dt == torch.int32 else FILL_F
            self.full[k] = torch.full((n + 1,) + shape, fill, dtype=dt, device=dev)

    def views(self):
        return {k: v[: self.n] for k, v in self.full.items()}

    def result(self):
        import torch

        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in self.full.items()}
        for k, v in out.items():
            assert (v[self.n] == (FILL_I if v.dtype == np.int32 else FILL_F)).all(), "%s: the slot past the batch was written" % k
        return {k: v[: self.n] for k, v in out.items()}


def _t(a, dtype=None):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))
    return t if dtype is None else t.to(dtype)


def _edges(run, n, keys, res):
    """The locality and batch-edge launches of a one-thread-per-race entry; run(idx) launches the races idx of the set."""
    p = _perm(n, 4)
    _same(run(p), res, keys, p, "permuted launch")
    tiled = np.arange(257) % n
    _same(run(tiled), res, keys, tiled, "257 races")
    for one in (0, n - 1):
        _same(run(np.array([one])), res, keys, np.array([one]), "a single race")


@pytest.mark.parametrize("N,V", [(10, 3), (12, 6)])
def test_track_prep(gpu, Z, N, V):
    import torch
    from crx import torch_api

    b = fc.track_batch(Z, N, V)
    N1 = N + 1

    def run(i):
        g = Guarded(len(i), dict(xt=((N1, 6), torch.float64), obs_s=((V, N1), torch.float64), obs_ey=((V, N1), torch.float64),
                                 lap_off=((V,), torch.float64), n_obs=((), torch.int32)))
        o = g.views()
        torch_api.track_prep_dev(N, V, b["L"], _t(b["x"][i]), _t(b["n_veh"][i]), _t(b["obs_s_in"][i]), _t(b["obs_ey_in"][i]), _t(b["traj"][i]),
                                 o["xt"], o["obs_s"], o["obs_ey"], o["lap_off"], o["n_obs"])
        return g.result()

    n = len(b["names"])
    res = run(np.arange(n))
    fc.check_track(res, b)
    _edges(run, n, fc.NLP_KEYS + ("xt",), res)


def _cbf_run(b, laps_entry):
    import torch
    from crx import torch_api

    N, V, N1 = b["N"], b["V"], b["N"] + 1

    def run(i):
        g = Guarded(len(i), dict(obs_s=((V, N1), torch.float64), obs_ey=((V, N1), torch.float64), lap_off=((V,), torch.float64), n_obs=((), torch.int32)))
        o = g.views()
        args = (b["t"], b["dt"], _t(b["x"][i]), _t(b["car_s0"][i]), _t(b["car_v"][i]), _t(b["car_ey"][i]), o["obs_s"], o["obs_ey"], o["lap_off"], o["n_obs"])
        if laps_entry:
            torch_api.cbf_prep_laps_dev(N, _t(b["lap"][i]), *args)
        else:
            assert (b["lap"] == b["lap"][0]).all()
            torch_api.cbf_prep_dev(N, float(b["lap"][0]), *args)
        return g.result()

    return run


@pytest.mark.parametrize("N,V", [(10, 3), (12, 6)])
def test_cbf_prep(gpu, Z, N, V):
    b = fc.cbf_batch(Z, N, (16,), V)
    run = _cbf_run(b, False)
    n = len(b["names"])
    res = run(np.arange(n))
    fc.check_cbf(res, b)
    _edges(run, n, fc.NLP_KEYS, res)


@pytest.mark.parametrize("N,V", [(10, 3), (12, 6)])
@pytest.mark.parametrize("laps", [(16,), (16, 32)], ids=["all16", "half32"])
def test_cbf_prep_laps(gpu, Z, N, V, laps):
    """Each race folds and offsets by its own lap length: all 16.0, then half of the launch on 32.0 with the edges of that lap."""
    b = fc.cbf_batch(Z, N, laps, V)
    n = len(b["names"])
    if len(laps) == 2:   # interleave the two laps, so that neighbouring threads fold by different lengths
        il = np.arange(n).reshape(2, n // 2).T.reshape(-1)
        for k in ("x", "car_s0", "car_v", "car_ey", "lap"):
            b[k] = b[k][il]
        b["names"], b["rec"] = [b["names"][j] for j in il], [b["rec"][j] for j in il]
        assert set(b["lap"][:2]) == {16.0, 32.0}
    run = _cbf_run(b, True)
    res = run(np.arange(n))
    fc.check_cbf(res, b)
    _edges(run, n, fc.NLP_KEYS, res)


@pytest.mark.parametrize("N,shape", [(10, (13, 1)), (12, (1, 13))])
def test_game_traffic(gpu, Z, N, shape):
    import torch
    from crx import torch_api

    b = fc.traffic_batch(Z, N, shape)
    N1 = N + 1

    def run(i, cars=shape[1]):
        """The races i of the set; with cars == 1 the set is taken car by car (13 races of one car)."""
        s0, v, ey = (b[k].reshape(-1, cars)[i] for k in ("s0", "v", "ey"))
        g = Guarded(len(i), dict(veh_xcurv=((cars, 6), torch.float64), pred_s=((cars, N1), torch.float64), pred_ey=((cars, N1), torch.float64)))
        o = g.views()
        torch_api.game_traffic_dev(N, b["L"], b["t"], b["dt"], _t(s0), _t(v), _t(ey), o["veh_xcurv"], o["pred_s"], o["pred_ey"])
        return {k: a.reshape((len(i) * cars,) + a.shape[2:]) for k, a in g.result().items()}

    res = run(np.arange(shape[0]))
    fc.check_traffic(res, b)
    one = lambda i: run(i, 1)   # noqa: E731
    _edges(one, 13, fc.TRAFFIC_KEYS, res)
