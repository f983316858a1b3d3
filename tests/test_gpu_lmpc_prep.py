"""crx_lmpc_prep_kernel and crx_lmpc_addpoint_kernel on the GPU (GPU box only) against the oracle and the numpy model
(tests/lmpcprep_model.py) on the crafted safe sets of tests/test_lmpcprep_model_cpu.py: that file's table says what each case reaches
and asserts, on the CPU, that it does.

Per call:
  status, safe-set points, cost-to-go          bit-exact against the oracle
  regression rows of well-posed stages         |kernel - oracle| <= 1e-12 max(1, |A|max of the stage)   (the figure of test_lmpc_prep_device)
  kinematic rows                               1e-13 (A), 1e-12 (C)
  stages that are not well-posed               every value finite (the status bit is part of the first line)
  singular stages                              the three regression rows of A, B, C are bitwise what the caller passed
  predictions of well-posed stages             against the model at helpers.LMPCPREP_PRED_TOL (measured in the CPU file)
  batch independence                           races [3:9] alone: the same bits
  masking                                      active = 0 on every third race: its outputs untouched, CRX_SKIPPED; the others unchanged"""
import numpy as np
import pytest

import helpers
import lmpcprep_model as M

pytestmark = pytest.mark.gpu

OUT = ("A", "B", "C", "ss", "qfun", "status")


@pytest.fixture(scope="module")
def gpu():
    import crx

    return crx.init(0)


def _kernel(gpu, case, rows=slice(None), seed=None):
    seed = helpers.lmpcprep_seed(case) if seed is None else seed
    args = case["args"]
    return gpu.lmpc_prep(helpers.lmpcprep_abi_desc(case["desc"]), *(a[rows] for a in args[:8]), args[8], from_plan=case["from_plan"],
                         seed=tuple(s[rows] for s in seed))


def check_call(gpu, orc, case):
    """The first six lines of the module docstring for one call -> the kernel's result."""
    ro, model = helpers.lmpcprep_reference(orc, case)
    rec, seed, label = model[6], helpers.lmpcprep_seed(case), case["name"]
    rg = _kernel(gpu, case)
    for k in ("status", "ss", "qfun"):
        np.testing.assert_array_equal(rg[k], ro[k], err_msg=label + " " + k)
    wp, sing = M.well_posed(rec), rec["singular"]
    scale = np.maximum(1.0, np.abs(ro["A"]).max(axis=(2, 3)))              # per stage
    for k in "ABC":
        dev = np.abs(rg[k][:, :, :3] - ro[k][:, :, :3]).reshape(scale.shape + (-1,)).max(axis=2) / scale
        print("%s %s: worst regression-row deviation from the oracle over well-posed stages %.3g (bound 1e-12)" % (label, k, dev[wp].max() if wp.any() else 0.0))
        assert (dev[wp] <= 1e-12).all(), (label, k, float(dev[wp].max()))
        assert np.isfinite(rg[k]).all(), (label, k)
        np.testing.assert_array_equal(rg[k][sing][:, :3], seed["ABC".index(k)][sing][:, :3], err_msg=label + ": rows of a singular stage, " + k)
    np.testing.assert_allclose(rg["A"][:, :, 3:], ro["A"][:, :, 3:], rtol=0, atol=1e-13, err_msg=label)
    np.testing.assert_allclose(rg["C"][:, :, 3:], ro["C"][:, :, 3:], rtol=0, atol=1e-12, err_msg=label)
    np.testing.assert_array_equal(rg["B"][:, :, 3:], 0.0, err_msg=label)
    worst = helpers.lmpcprep_compare_with_model(rg, model, case, label)
    print("%s: worst prediction deviation from the model %.3g (bound %.3g)" % (label, worst, helpers.LMPCPREP_PRED_TOL))
    return rg


def test_case_g_lds_attribute_raised(gpu, orc):
    """a, b, a in one process: b needs more dynamic LDS than a (the attribute is raised between the calls), and the smaller call is
    still right, to the bit what it was, afterwards.  First in the file: a smaller call comes before b when the file runs alone.
    crx_launch_lmpcprep keeps the size it last set in a static, so the raise between a and b happens here only if no earlier prep call of
    the process used a table of b's size or more: in the whole suite that holds because b's n_points = 1100 is the largest any test
    uses (the recorded racing game has 600) -- a new test with a larger table, collected before this file, would move the raise there."""
    a, b = helpers.lmpcprep_cases()["a"][0], helpers.lmpcprep_cases()["b"][0]
    assert b["desc"].n_points > a["desc"].n_points
    first = check_call(gpu, orc, a)
    check_call(gpu, orc, b)
    again = check_call(gpu, orc, a)
    for k in OUT:
        np.testing.assert_array_equal(again[k], first[k], err_msg=k)


@pytest.mark.parametrize("name", helpers.LMPCPREP_CASE_NAMES)
def test_kernel_against_oracle_and_model(gpu, orc, name):
    for case in helpers.lmpcprep_cases()[name]:
        rg = check_call(gpu, orc, case)
        sub = _kernel(gpu, case, rows=slice(3, 9))
        for k in OUT:
            np.testing.assert_array_equal(sub[k], rg[k][3:9], err_msg=case["name"] + ": races [3:9] alone, " + k)


@pytest.mark.parametrize("name", helpers.LMPCPREP_CASE_NAMES)
def test_masked_launch(gpu, orc, name):
    import torch

    from crx import abi, torch_api

    dev = torch.device("cuda", 0)
    for case in helpers.lmpcprep_cases()[name]:
        d, args, Bn = helpers.lmpcprep_abi_desc(case["desc"]), case["args"], len(case["args"][4])
        rg = _kernel(gpu, case)
        t = [torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in args]
        ws = torch_api.LmpcPrepWorkspace(d, Bn, dev)
        rng = np.random.default_rng(9)
        start = dict(zip("ABC", helpers.lmpcprep_seed(case)), ss=rng.normal(size=tuple(ws.ss.shape)), qfun=rng.normal(size=tuple(ws.qfun.shape)),
                     status=np.full(Bn, -7, dtype=np.int32))
        for k, v in start.items():
            getattr(ws, k).copy_(torch.as_tensor(v.reshape(tuple(getattr(ws, k).shape)), device=dev))
        active = (np.arange(Bn) % 3 != 0).astype(np.int32)
        torch_api.lmpc_prep_dev(d, *t, case["from_plan"], ws=ws, active=torch.as_tensor(active, device=dev))
        torch.cuda.synchronize(dev)
        on = active != 0
        for k in OUT:
            got = getattr(ws, k).cpu().numpy().reshape(rg[k].shape)
            np.testing.assert_array_equal(got[on], rg[k][on], err_msg=case["name"] + ": active races, " + k)
            if k == "status":
                assert (got[~on] == abi.CRX_SKIPPED).all(), got
            else:
                np.testing.assert_array_equal(got[~on], start[k].reshape(rg[k].shape)[~on], err_msg=case["name"] + ": masked races, " + k)


@pytest.mark.parametrize("u_stride", [2, 5])
def test_addpoint(gpu, orc, u_stride):
    """crx_lmpc_addpoint_dev against crx_oracle_lmpc_addpoint and the model: every byte of both tables, the untouched ones included
    (iter 0 .. L+1, rows P-2, P-1, P and negative: tests/test_lmpcprep_model_cpu.py asserts the draw holds them)."""
    import torch

    from crx import torch_api

    dev = torch.device("cuda", 0)
    case = M.make_addpoint(40 + u_stride, u_stride)
    d = case["desc"]
    ss_m, us_m = M.addpoint_model(d, case["ss"], case["us"], case["time_ss"], case["it"], case["step"], case["x"], case["u"], u_stride)
    ss_o, us_o, _ = helpers.lmpcprep_oracle_addpoint(orc, case)
    t = {k: torch.as_tensor(np.ascontiguousarray(case[k]), device=dev) for k in ("ss", "us", "time_ss", "it", "step", "x", "u")}
    torch_api.lmpc_addpoint_dev(helpers.lmpcprep_abi_desc(d), t["ss"], t["us"], t["time_ss"], t["it"], t["step"], t["x"], t["u"], u_stride)
    torch.cuda.synchronize(dev)
    ss_g, us_g = t["ss"].cpu().numpy(), t["us"].cpu().numpy()
    assert (ss_m != case["ss"]).any() and (us_m != case["us"]).any()
    for got, orc_, mod, k in ((ss_g, ss_o, ss_m, "ss"), (us_g, us_o, us_m, "us")):
        np.testing.assert_array_equal(got, orc_, err_msg=k + " against the oracle")
        np.testing.assert_array_equal(got, mod, err_msg=k + " against the model")
