"""The oracle of the learning-MPC prep (oracle/crx_oracle_lmpc_prep.c) against the independent numpy model (tests/lmpcprep_model.py) on
crafted safe sets, and the assertions that those inputs reach the data-dependent branches of crx_lmpc_prep_kernel they were made for
(tests/test_gpu_lmpc_prep.py runs the kernel on the same calls).  No GPU.

  case  shape                                                        reaches
  a     N=5, P=160, L=4, iter 2..4, laps 70..150, k=40, 30 % dups    laps other than 0/1, N not a multiple of 4, ties at the k-th distance
  b     N=7, P=1100, L=3, laps 700..1090, k=64, dups                 the LDS-keyed bisection (n > 512), k at its limit, ties across 64-lane chunks
  c     as a, N=6, bandwidth 0.74                                    partial / empty sets, partial next to top-k, singular stages (status 1)
  d     N=2 and N=3, P=96, k=8, given points and from_plan           waves without a stage
  e     laps of 20 and 500 / 513 samples in P=520, both orders       the feature-table stride, n = 19, 499 and exactly 512
  f     N=2, n_ss_per_lap 1/7/22/30 x n_ss_laps 1/2 x shift -5/0/3   first minimum among lanes, first + shift < 0, the clamp to the last row
  g     a, b, a                                                      (on the GPU: the dynamic-LDS attribute raised between calls)

Comparison: status, safe-set points and cost-to-go exactly; kinematic rows to 1e-13 (A) and 1e-12 (C); regression rows as PREDICTIONS
A[:3] x + B[:3] u + C[:3] at the stage's own linearisation point, over the well-posed stages (at least 10 selected samples, condition
estimate at most 1e12) -- the coefficients of an ill-posed stage are not comparable between two routes, the prediction is."""
import math

import numpy as np
import pytest

import helpers
import lmpcprep_model as M

# The measurement behind the prediction tolerance (test_prediction_deviation repeats and prints it): the largest |oracle - model| of a
# prediction over all well-posed stages of all calls below is 1.23e-13 (1265 stages); the tolerance is ten times that, rounded up to one
# digit: 2e-12.  The two figures are defined once, next to the comparison both test files use (tests/helpers.py), and named here.
PRED_DEV_MEASURED = helpers.LMPCPREP_PRED_DEV_MEASURED
PRED_TOL = helpers.LMPCPREP_PRED_TOL
CASE_NAMES = helpers.LMPCPREP_CASE_NAMES
ILL_POSED_SHARE = dict(a=0.0, b=0.0, c=0.25, d=0.0, e=0.0, f=0.0)
compare_with_model, oracle_addpoint = helpers.lmpcprep_compare_with_model, helpers.lmpcprep_oracle_addpoint


def _calls(name):
    return helpers.lmpcprep_cases()[name]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_against_model(orc, name):
    for case in _calls(name):
        ro, model = helpers.lmpcprep_reference(orc, case)
        rec, seed = model[6], helpers.lmpcprep_seed(case)
        compare_with_model(ro, model, case, case["name"])
        # a singular stage keeps the three regression rows the caller passed, in the oracle and in the model alike
        for k, m, s in zip("ABC", model[:3], seed):
            np.testing.assert_array_equal(ro[k][rec["singular"]][:, :3], s[rec["singular"]][:, :3], err_msg=case["name"] + k)
            np.testing.assert_array_equal(m[rec["singular"]][:, :3], s[rec["singular"]][:, :3], err_msg=case["name"] + k)
        # between "nothing selected" and "enough different rows", whether elimination meets an exact zero is rounding: no such stage
        assert not ((rec["distinct"] > 0) & (rec["distinct"] < 8)).any(), case["name"]
        assert (rec["singular"] == (rec["total"] == 0)).all(), case["name"]
        ill = 1.0 - M.well_posed(rec).mean()
        assert ill <= ILL_POSED_SHARE[name], (case["name"], ill)


def test_case_g_sequence(orc):
    """a, b, a run one after the other give what each gives alone (the oracle keeps no state between calls)."""
    a, b = _calls("a")[0], _calls("b")[0]
    for case in (a, b, a):
        ref = helpers.lmpcprep_reference(orc, case)[0]
        ro = orc.lmpc_prep(helpers.lmpcprep_abi_desc(case["desc"]), *case["args"], from_plan=case["from_plan"], seed=helpers.lmpcprep_seed(case))
        for k in ref:
            np.testing.assert_array_equal(ro[k], ref[k], err_msg=case["name"] + k)


def test_prediction_deviation(orc):
    """The measurement behind PRED_TOL, repeated: the largest oracle-against-model deviation over all well-posed stages."""
    worst, stages = 0.0, 0
    for name in CASE_NAMES:
        for case in _calls(name):
            ro, model = helpers.lmpcprep_reference(orc, case)
            worst = max(worst, compare_with_model(ro, model, case, case["name"], tol=np.inf))
            stages += int(M.well_posed(model[6]).sum())
    print("largest |oracle - model| prediction deviation over %d well-posed stages: %.3g (recorded %.3g, tolerance %.3g)"
          % (stages, worst, PRED_DEV_MEASURED, PRED_TOL))
    assert worst <= PRED_TOL, worst
    # the rule the tolerance was set by: ten times the recorded measurement, rounded up to one digit
    digit = 10.0 ** math.floor(math.log10(10 * PRED_DEV_MEASURED))
    assert math.isclose(PRED_TOL, math.ceil(10 * PRED_DEV_MEASURED / digit) * digit, rel_tol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- reach
def _rec(orc, name):
    return [helpers.lmpcprep_reference(orc, case)[1][6] for case in _calls(name)]


def test_reach_a(orc):
    (rec,), (case,) = _rec(orc, "a"), _calls("a")
    assert (rec["arm"] == M.TOP).all()
    assert rec["tie"].sum() >= 20, rec["tie"].sum()
    assert set(case["args"][4].tolist()) == {2, 3, 4}
    assert case["desc"].N % 4 != 0


def test_reach_b(orc):
    (rec,), (case,) = _rec(orc, "b"), _calls("b")
    assert (rec["n"] > 512).all() and (rec["arm"] == M.TOP).all() and case["desc"].max_neighbours == 64
    assert rec["tie"].sum() >= 20, rec["tie"].sum()
    assert (rec["tie"] & (rec["tie_span"] > 64)).sum() >= 5


def test_reach_c(orc):
    (rec,), (case,) = _rec(orc, "c"), _calls("c")
    status = helpers.lmpcprep_reference(orc, case)[1][5]
    for arm in (M.TOP, M.PARTIAL, M.EMPTY):
        assert (rec["arm"] == arm).mean() >= 0.10, (arm, (rec["arm"] == arm).mean())
    mixed = (rec["arm"] == M.TOP).any(axis=2) & (rec["arm"] == M.PARTIAL).any(axis=2)
    assert mixed.sum() >= 5, mixed.sum()
    assert (status == 1).sum() >= 3 and (status == 0).sum() >= 3, status
    assert rec["inside"].min() == 0 and 40 <= rec["inside"].max() <= 60, (rec["inside"].min(), rec["inside"].max())
    part = rec["count"][rec["arm"] == M.PARTIAL]
    assert part.min() >= 1 and part.max() < case["desc"].max_neighbours


def test_reach_d(orc):
    calls = _calls("d")
    assert sorted((c["desc"].N, c["from_plan"]) for c in calls) == [(2, False), (2, True), (3, False), (3, True)]
    assert all(c["desc"].n_points == 96 and c["desc"].max_neighbours == 8 for c in calls)


def test_reach_e(orc):
    (rec,), (case,) = _rec(orc, "e"), _calls("e")
    assert case["desc"].n_points == 520
    assert set(rec["n"].ravel().tolist()) == {19, 499, 512}
    n = rec["n"][:, 0]                                                 # (lap iter-2, lap iter-1) of every race
    orders = {(int(p), int(q)) for p, q in n}
    assert {(19, 499), (499, 19), (19, 512), (512, 19)} <= orders, orders


def test_reach_f(orc):
    recs, calls = _rec(orc, "f"), _calls("f")
    assert {(c["desc"].n_ss_per_lap, c["desc"].n_ss_laps, c["desc"].shift) for c in calls} == {(a, b, s) for a in (1, 7, 22, 30) for b in (1, 2) for s in (-5, 0, 3)}
    tie = sum(int((r["near_tie"] & (r["near_span"] > 64)).any(axis=1).sum()) for r in recs)
    clamp = sum(int(r["clamp"].any(axis=1).sum()) for r in recs)
    neg = sum(int(r["neg"].any(axis=1).sum()) for r in recs)
    assert tie >= 5 and clamp >= 5 and neg >= 5, (tie, clamp, neg)
    # a tie whose later row sits in a LOWER lane of the wave than the first one, and one in the same lane
    lower = same = 0
    for r, c in zip(recs, calls):
        ss, it, x = c["args"][0], c["args"][4], c["args"][5]
        for b, jj in zip(*np.nonzero(r["near_tie"])):
            norm = np.abs(ss[b, it[b] - jj - 1] - x[b]).sum(axis=1)
            at = np.flatnonzero(np.isclose(norm, norm.min(), rtol=0, atol=1e-12))
            lower += int((at[1:] % 64 < at[0] % 64).any())
            same += int((at[1:] % 64 == at[0] % 64).any())
    assert lower >= 3 and same >= 3, (lower, same)


# ------------------------------------------------------------------------------------------------------------- add_point
@pytest.mark.parametrize("u_stride", [2, 5])
def test_addpoint_oracle_against_model(orc, u_stride):
    case = M.make_addpoint(40 + u_stride, u_stride)
    d, L, P = case["desc"], case["desc"].n_laps, case["desc"].n_points
    ss_m, us_m = M.addpoint_model(d, case["ss"], case["us"], case["time_ss"], case["it"], case["step"], case["x"], case["u"], u_stride)
    ss_o, us_o, rc = oracle_addpoint(orc, case)
    np.testing.assert_array_equal(ss_o, ss_m)
    np.testing.assert_array_equal(us_o, us_m)
    lap_ok = (case["it"] >= 1) & (case["it"] <= L)
    assert ((rc == 0) == lap_ok).all(), rc                            # the oracle refuses a lap outside the table; the kernel skips it
    # reach: every iter 0 .. L+1, rows P-2, P-1 (written), P and negative ones (skipped)
    assert set(case["it"].tolist()) == set(range(L + 2))
    row = np.array([case["time_ss"][b, min(max(case["it"][b] - 1, 0), L - 1)] + case["step"][b] + 1 for b in range(len(rc))])
    assert {P - 2, P - 1, P, -1} <= set(row[lap_ok].tolist()), sorted(set(row[lap_ok].tolist()))
    changed = (ss_m != case["ss"]).any(axis=(1, 2, 3))
    assert (changed == (lap_ok & (row >= 0) & (row < P))).all()
