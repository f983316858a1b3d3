"""The CPU side of the front-end kernels, held to what the reference decides exactly on the edges of its comparisons.

tests/golden/front_edges.npz (tests/golden/tools/make_front_edges.py) records the reference's own interest test, partial sort,
Bezier end point, ey windows, region selection, obstacle windows, per-stage targets and scripted cars with the deciding quantity
exactly ON its edge and one np.nextafter to either side.  Held to it here, case by case: tests/front_model.py (the plain model the
GPU tests use as their second reference), crx.hostprep, planning.planner_helper and the CPU oracle's planner_scene and select (the
oracle has no planner_prep: the Bezier and ey-bound stage is held through planner_helper and hostprep).  Decisions, integers and
copies bit for bit; Bezier polylines to 1e-14, per-stage targets to 1e-13.

Cases per stage and pinned comparison, as the generator prints them (`(exact)` / `(all)` rows count the exact-arithmetic pins, one
per evaluated comparison; the others count cases):

    bezier      middle_region_between_two 2, raw_state_copied_not_wrapped 2, s3==L:s3>=L 12, s_end==opt_s[0]:s_end<=opt_s[0] 6,
                s_end_on_interior_node:xs[hi]<x 6; s3>=L(exact) 24, s_end<=opt_s[0](exact) 24
    ey_window   s_nom==os-win:left_and_right 6, s_nom==os-win:stage0_only 6, s_nom==os+win:left_and_right 6,
                s_nom==os+win:stage0_only 6, both_neighbours_inside:fmax 4, prediction_at_L_not_wrapped:os>L 2,
                prediction_at_L_plus_half_wraps:os>L 2, prediction_ulp_above_L_wraps:os>L 2; s_nom>=os-win 836, s_nom<=os+win 836
    interest    c1_dist 6, c2_dist 6, c3_dist 6, c4_dist 6, c1c3_order:s_a==s_e 6, c2_order:s_a+L==s_e 6, c4_order:s_a==s_e+L 6,
                ego_at_L_not_wrapped:c2_dist 6, ego_nextafter_L_wraps:c1_dist 6, agent_at_L_not_wrapped:c1_dist 6,
                agent_at_L_not_wrapped:c3_order 6
    overflow    (no recorded answer) equidistant_ahead_behind 1, equidistant_behind_ahead 1, equidistant_across_line 1,
                equidistant_across_line_rev 1, two_dropped:overflow_counts 1, all_equidistant:first_kept 1,
                eight_around_six_slots 1, seven_around_six_slots:equidistant_last 1
    select      circle:h>=0 74 (exact), equal_cost:first_wins 14, switch_penalty:old!=r 10, nan_point_is_hit 4, inf_point_is_no_hit 4,
                prediction_at_L_not_wrapped:os>L 4, prediction_at_L_plus_half_wraps:os>L 4
    sort        equal_ey_goes_front:e>=first 12, ulp_above_first_goes_front 2, ulp_below_first_goes_back 2,
                veh_info_in_iteration_order 2, max_dv_equal_speeds:fmax 4
    target      first_node:s<s_lo 10, last_node:s>=s_hi 6, interior_node:xs[hi]<x 8, clipped_below_first 4, clipped_above_last 2
    traffic     lands_at_L:s>L 4, lands_at_2L:ceil(s_over_L)-1 2, between_L_and_2L 2, v==0 3, before_the_line 1, negative_s 1
    window      lower:dist_ego>dist_obs-margin 48, upper:dist_ego<dist_obs+margin 36, ego_at_L:int(s_over_L) 8, ego_at_2L 8,
                obstacle_at_L 8, obstacle_negative_s:int()_toward_zero 12, packing 20; all other evaluated comparisons 420 (exact)
    cases       interest 66, overflow 8, plan10 71, plan12 71, target10 15, target12 15, traffic 13, win{10,12}_{16,32} 21 each
"""
import types

import numpy as np
import pytest

import front_edges_cases as fc
import front_model as fm


@pytest.fixture(scope="module")
def Z():
    return fc.load()


NS = types.SimpleNamespace


@pytest.mark.parametrize("N,VA,V", [(10, 6, 3), (12, 8, 6)])
def test_scene_model_and_oracle(Z, orc, N, VA, V):
    from crx import abi

    b = fc.scene_batch(Z, N, VA, V)
    model = fc.scene_model(b)
    fc.check_scene(model, b, model)
    d = abi.scene_desc(N, VA, V, b["L"], veh_length=b["length"])
    fc.check_scene(orc.planner_scene(d, b["ego"], b["n_all"], b["veh"], b["pred_s"], b["pred_ey"]), b, model)
    # the library's own policy, spelled out for the crafted ties: the EARLIER of two equidistant candidates stays
    for i, nm in enumerate(b["names"]):
        if "norecord/equidistant" in nm:
            assert list(model["order"][i][model["order"][i] >= 0]) and 0 in model["order"][i] and 3 not in model["order"][i], nm
            assert model["overflow"][i] == 1 and model["n_veh"][i] == V, nm
        if "two_dropped" in nm:
            assert model["overflow"][i] == 2, nm
    assert any("overflow/" in nm for nm in b["names"])


def test_interest_and_sort_mirror(Z):
    from planning import planner_helper as ph

    L, par = float(Z["L"]), NS(safety_factor=4.5, planning_prediction_factor=0.5)
    mk = lambda v, s: NS(xcurv=np.array([v, 0, 0, 0, s, 0.0]), param=NS(length=float(Z["length"]), width=float(Z["width"])))   # noqa: E731
    it = fc.group(Z, "interest")
    for i, nm in enumerate(it["names"]):
        got = ph.check_ego_agent_distance(mk(it["ego_v"][i], it["ego_s"][i]), mk(it["agent_v"][i], it["agent_s"][i]), par, L)
        assert got == bool(it["want"][i]), nm
        assert fm.interest(it["ego_v"][i], it["ego_s"][i], it["agent_v"][i], it["agent_s"][i], L, float(Z["length"])) == bool(it["want"][i]), nm
    for N in (10, 12):
        pl = fc.group(Z, "plan%d" % N)
        for i, nm in enumerate(pl["names"]):
            hit = [int(v) for v in np.nonzero(pl["interest"][i])[0]]
            order = ph.sort_by_ey(hit, lambda v: pl["veh"][i, v, 5])
            assert order == list(pl["order"][i, :len(hit)]), nm
            vehicles = {"ego": NS(xcurv=pl["x_raw"][i]), **{v: NS(xcurv=pl["veh"][i, v]) for v in hit}}
            assert ph.get_agent_info(vehicles, order, NS(lap_length=L)).max_delta_v == pl["max_dv"][i], nm


@pytest.mark.parametrize("N", [10, 12])
def test_prep_model_and_mirror(Z, N):
    from crx import hostprep
    from planning import planner_helper as ph

    b = fc.prep_batch(Z, N, 6)
    model = fc.prep_model(b)
    fc.check_prep(model, b, model)
    for i, nm in enumerate(b["names"]):   # the recorded windows, decision by decision
        nv = b["rec"][i]["nv"]
        np.testing.assert_array_equal(model["active"][i, :nv + 1], b["rec"][i]["active"], err_msg=nm)
    opt = np.zeros((len(b["opt_s"]), 6))
    opt[:, 4], opt[:, 5] = b["opt_s"], b["opt_ey"]
    lb, ub = hostprep.planner_ey_bounds(b["x_wrapped"], b["obs_s"], b["obs_ey"], b["n_veh"], b["track_width"], b["L"], N, veh_length=b["length"],
                                        veh_width=b["width"])
    for i, nm in enumerate(b["names"]):
        nv = b["rec"][i]["nv"]
        cp = ph.bezier_control_points(nv, b["veh_info"][i, :nv], b["max_dv"][i], 0.5, b["track_width"], b["L"], b["width"], opt, b["x_wrapped"][i])
        np.testing.assert_allclose(ph.bezier_polylines(cp, N), b["rec"][i]["bez"], rtol=0, atol=fc.BEZ_TOL, err_msg=nm)
        np.testing.assert_array_equal(lb[i, :nv + 1], fc.lb_from_active(b, i, b["rec"][i]["active"]), err_msg=nm)
        np.testing.assert_array_equal(ub[i], model["ey_ub"][i], err_msg=nm)
    # wrap_above against the reference's loop at the edge
    s = np.array([b["L"], np.nextafter(b["L"], 0), np.nextafter(b["L"], 99), 2 * b["L"], np.nextafter(2 * b["L"], 99), b["L"] + 0.5, 0.0, -4.0])
    np.testing.assert_array_equal(hostprep.wrap_above(s, b["L"]), [fm.wrap_above(float(v), b["L"]) for v in s])


@pytest.mark.parametrize("N,V", [(10, 3), (12, 6)])
def test_select_model_and_oracle(Z, orc, N, V):
    from crx import abi

    b = fc.select_batch(Z, N, V)
    model = fc.select_model(b)
    fc.check_select(model, b, model)
    d = abi.select_desc(N, V, b["L"], veh_length=b["length"], veh_width=b["width"])
    fc.check_select(orc.select(d, b["n_veh"], b["X"], b["obs_s"], b["obs_ey"], b["old_flag"]), b, model)


@pytest.mark.parametrize("N", [10, 12])
def test_windows_and_targets_model_and_mirror(Z, N):
    from crx import hostprep

    for laps in ((16,), (16, 32)):
        b = fc.cbf_batch(Z, N, laps)
        model = fc.cbf_model(b)
        fc.check_cbf(model, b, model)
        for i, nm in enumerate(b["names"]):
            ps = np.array([[b["car_v"][i, v] * (b["t"] + j * b["dt"]) + b["car_s0"][i, v] for j in range(N + 1)] for v in range(3)])
            pe = np.tile(b["car_ey"][i][:, None], (1, N + 1))
            keep, off = hostprep.cbf_window(b["x"][i:i + 1], ps[None, :, 0], b["lap"][i])
            s, e, o, n = hostprep.pack_obstacles(keep, ps[None], pe[None], off, 3)
            fc._check_packed(dict(obs_s=s, obs_ey=e, lap_off=o, n_obs=n), 0, nm, b["rec"][i], 3)
    b = fc.track_batch(Z, N)
    model = fc.track_model(b)
    fc.check_track(model, b, model)
    for i, nm in enumerate(b["names"]):
        nv = int(b["n_veh"][i])
        np.testing.assert_allclose(hostprep.tracking_targets(b["x"][i], b["traj"][i], N), model["xt"][i], rtol=0, atol=fc.TARGET_TOL, err_msg=nm)
        if "xt_ey" in b["rec"][i]:
            np.testing.assert_allclose(hostprep.tracking_targets(b["x"][i], b["traj"][i], N)[:, 5], b["rec"][i]["xt_ey"], rtol=0, atol=fc.TARGET_TOL, err_msg=nm)
        if nv:
            keep, off = hostprep.cbf_window(b["x"][i:i + 1], b["obs_s_in"][i:i + 1, :nv, 0], b["L"])
            s, e, o, n = hostprep.pack_obstacles(keep, b["obs_s_in"][i:i + 1, :nv], b["obs_ey_in"][i:i + 1, :nv], off, 3)
            fc._check_packed(dict(obs_s=s, obs_ey=e, lap_off=o, n_obs=n), 0, nm, b["rec"][i], 3)


def test_traffic_model(Z):
    for N in (10, 12):
        b = fc.traffic_batch(Z, N, (13, 1))
        model = fc.traffic_model(b)
        fc.check_traffic(model, b, model)
