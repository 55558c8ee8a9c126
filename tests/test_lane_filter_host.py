"""vp_lanes without a GPU: the ABI, the numpy twin against literal expectations for the hand-made cases, and the host fit vp_lanes_fit (the library's own
host code, no device) against the exact rational solution on every fitted lane of the generated set.

What stays unpinned: the reference solves the same least-squares problem with cv::solve(DECOMP_SVD) in double.  OpenCV is not available to these tests,
so how far ITS rounding lies from the exact solution is not measured here; numpy.linalg.lstsq (LAPACK's SVD driver) stands in as the sanity check that
the normal equations built from the integer moments are the problem an SVD solves."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import abi  # noqa: E402
import lane_filter_cases as lc  # noqa: E402
import lane_filter_ref as ref  # noqa: E402

# the worst distance, over rows 0 .. 79 and every fitted lane of the generated and hand-made sets, between the curve of the exact solution and the
# curve numpy.linalg.lstsq gives for the same points: measured 1.476e-10 px where this was written; the bar is 100 times the measurement
LSTSQ_MEASURED_PX = 1.476e-10
LSTSQ_BAR_PX = 100 * LSTSQ_MEASURED_PX


def fitted_lanes():
    """(points, twin lane) of every lane with a fit or a singular system, hand-made cases included"""
    _, results, _, _ = lc.generated()
    out = [r for res in results for r in res]
    out += [r for k in lc.HAND_NAMES for r in ref.LaneFilterRef().update(*lc.HAND[k])]
    return [r for r in out if r["order"] or r["singular"]]


# ---- the ABI
def test_new_symbols_are_declared_exported_and_bound_and_the_structs_match():
    from autoware_vision_pilot_amd import lib

    src = abi.header_source()
    declared, exported = abi.declared_symbols(), abi.exported_symbols()
    for s in lc.NEW_SYMBOLS:
        assert s in declared and s in exported and s in lib.EXPORTED_SYMBOLS and s in lib._SIGS, s
    assert {s for s in declared if s.startswith("vp_lanes_")} == set(lc.NEW_SYMBOLS) == {s for s in lib._SIGS if s.startswith("vp_lanes_")}
    assert {s for s in exported if s.startswith("vp_lanes_")} == set(lc.NEW_SYMBOLS)
    assert all(s.startswith("vp_") for s in exported)
    assert "#define VP_LANES_MAX_WINDOWS 40" in src and "#define VP_LANES_MAX_POINTS 1920" in src
    assert "enum vp_lanes_flags { VP_LANES_SINGULAR = 1, VP_LANES_SMOOTHED = 2 };" in src
    assert (lib.VP_LANES_MAX_WINDOWS, lib.VP_LANES_MAX_POINTS, lib.VP_LANES_SINGULAR, lib.VP_LANES_SMOOTHED) == (40, 1920, 1, 2)
    assert "int16_t windows[VP_LANES_MAX_WINDOWS][4];" in src and "double raw_coeffs[6], coeffs[6];" in src and "int64_t S[5], T[3];" in src
    D = lib.LANES_LANE_DTYPE
    assert D.itemsize == 528 and lib.LANES_RESULT_DTYPE.itemsize == 1056
    for name, off in (("start_x", 0), ("n_windows_up", 8), ("n_points_up", 16), ("min_y", 24), ("S", 32), ("T", 72), ("windows", 96), ("order", 416), ("flags", 420),
                      ("coeffs_valid", 424), ("raw_coeffs", 432), ("coeffs", 480)):
        assert D.fields[name][1] == off, name
    # the older records are as they were
    assert ct.sizeof(lib.MetricFrame) == 72 and ct.sizeof(lib.MetricLanesFrame) == 96


# ---- the twin
@pytest.mark.parametrize("name", lc.HAND_NAMES)
def test_twin_against_literal_expectations(name):
    got = tuple(lc.lane_tuple(r) for r in ref.LaneFilterRef().update(*lc.HAND[name]))
    assert got == lc.EXPECT[name]


def test_twin_details_of_the_hand_made_cases():
    up = ref.LaneFilterRef().update(*lc.HAND["top_clip"])[0]
    assert up["windows_up"][0] == (64, 36, 12, 4) and up["windows_up"][1] == (69, 34, 2, 4)      # half-width 6 at y = 40, 1 above
    assert up["windows_up"][-1] == (69, 0, 2, 2)                                                   # the window the top clips
    assert up["windows_down"] == [(64, y, 12, 4) for y in range(44, 80, 4)]
    left, right = ref.LaneFilterRef().update(*lc.HAND["edges"])
    assert left["windows_up"][0] == (0, 75, 6, 4) and right["windows_up"][0] == (153, 75, 7, 4)  # [x - 6, x + 6) clipped to the plane
    br = ref.LaneFilterRef().update(*lc.HAND["bridged_below"])[0]
    assert {p for p in br["points_up"] if 58 <= p[1] <= 69} == {(50, y) for y in range(58, 70)}    # the ego gap, filled from the other-lane plane
    un = ref.LaneFilterRef().update(*lc.HAND["unbridged_above"])[0]
    assert not [p for p in un["points_up"] if 28 <= p[1] <= 36] and [p for p in un["points_up"] if 37 <= p[1] <= 39] == [(50, 37), (50, 38), (50, 39)]
    two = ref.LaneFilterRef().update(*lc.HAND["two_lines"])[0]
    assert two["points_up"][:8] == [(60, 75), (60, 76), (60, 77), (60, 78), (60, 73), (60, 74), (60, 75), (60, 76)]   # row-major, duplicates kept
    assert two["S"][0] == 75 and two["T"][0] == 60 * 75 and (two["min_y"], two["max_y"]) == (40, 78)
    sp = ref.LaneFilterRef().update(*lc.HAND["special_values"])[0]
    assert (60, 70) not in sp["points_up"] and (61, 78) not in sp["points_up"]                     # -inf is clear; the start pixel lies in no window


def test_smoothing_rules_of_the_twin():
    t = ref.LaneFilterRef(0.5)
    seq = [t.update(*lc.HAND[k]) for k in lc.SEQUENCE]
    assert [r[0]["smoothed"] for r in seq] == [False, True, False, False, False, True] and [r[1]["smoothed"] for r in seq] == [False, True, False, False, False, False]
    assert seq[1][0]["coeffs"] == [0.0, 0.0, 0.0, 65.0, 20.0, 58.5]      # (60, 40, 78) and (70, 0, 39) halved
    assert seq[2][0]["coeffs"] is None and seq[4][0]["coeffs"] is None and seq[4][0]["start"] == (60, 79)
    assert seq[5][0]["coeffs"] == [0.0, 0.0, 0.0, 30.0, 40.0, 78.0] and seq[5][1]["coeffs"] == [0.0, 0.0, 0.0, 100.0, 40.0, 78.0]
    t.reset()
    assert t.update(*lc.HAND["two_lines"])[0]["smoothed"] is False


# ---- the host fit
def test_fit_is_within_one_ulp_of_the_exact_solution_and_flags_exactly_the_singular_systems():
    """exact integer determinants, one rounded quotient: the bar is one ulp of the correctly rounded value"""
    from autoware_vision_pilot_amd import lib

    lanes = fitted_lanes()
    orders = [r["order"] for r in lanes]
    assert orders.count(1) >= 20 and orders.count(2) >= 20 and sum(r["singular"] for r in lanes) >= 1
    for r in lanes:
        n = r["S"][0]
        order = 1 if n < 30 else 2
        got, singular = lib.lanes_fit(r["S"], r["T"], order)
        assert singular == r["singular"], (r["S"], r["T"])
        if singular:
            assert got == (0.0, 0.0, 0.0)                            # out is left as the caller had it
            continue
        for g, ex in zip(got, r["exact"]):
            w = float(ex)
            assert abs(g - w) <= lc.ulp(w), (g, w)


@pytest.mark.parametrize("rows,order,singular", [((7,), 1, True), ((7, 9), 1, False), ((7, 9), 2, True), ((7, 9, 30), 2, False), ((0,), 1, True), ((0, 79), 2, True),
                                                 ((0, 1, 79), 2, False)])
def test_fit_singular_exactly_when_too_few_distinct_rows(rows, order, singular):
    from autoware_vision_pilot_amd import lib

    pts = [(40 + 3 * k + y % 5, y) for k in range(4) for y in rows]
    S, T = ref.moments(pts)
    got, flag = lib.lanes_fit(S, T, order)
    assert flag == singular and (ref.fit_exact(S, T, order) is None) == singular
    if not singular:
        for g, ex in zip(got, ref.fit_exact(S, T, order)):
            assert abs(g - float(ex)) <= lc.ulp(float(ex))


def test_fit_rounds_correctly_at_the_extremes():
    """quotients far from 1: the largest production moments (1920 points on row 79 and two more rows) and a tiny coefficient"""
    from autoware_vision_pilot_amd import lib

    pts = [(159, 79)] * 1900 + [(0, 78)] * 10 + [(1, 0)] * 10
    S, T = ref.moments(pts)
    assert max(S) < 1 << 40
    got, flag = lib.lanes_fit(S, T, 2)
    assert not flag
    for g, ex in zip(got, ref.fit_exact(S, T, 2)):
        assert abs(g - float(ex)) <= lc.ulp(float(ex)), (g, float(ex))
    pts = [(80, y) for y in range(0, 80)] + [(81, 79)]
    S, T = ref.moments(pts)
    got, _ = lib.lanes_fit(S, T, 2)
    for g, ex in zip(got, ref.fit_exact(S, T, 2)):
        assert abs(g - float(ex)) <= lc.ulp(float(ex)), (g, float(ex))


def test_the_normal_equations_are_the_least_squares_problem_an_svd_solves():
    ys = np.arange(80, dtype=np.float64)
    worst = 0.0
    for r in fitted_lanes():
        if not r["order"]:
            continue
        pts = np.array(r["points_up"] + r["points_down"], dtype=np.float64)
        y, x = pts[:, 1], pts[:, 0]
        A = np.stack([y * y, y, np.ones_like(y)], axis=1)[:, 3 - (r["order"] + 1):]
        sol = np.linalg.lstsq(A, x, rcond=None)[0]
        abc = np.concatenate([np.zeros(3 - sol.size), sol])
        ex = [float(v) for v in r["exact"]]
        d = np.abs((abc[0] - ex[0]) * ys * ys + (abc[1] - ex[1]) * ys + (abc[2] - ex[2])).max()
        worst = max(worst, float(d))
    print("worst curve distance from numpy.linalg.lstsq over rows 0 .. 79: %.3e px (bar %.1e)" % (worst, LSTSQ_BAR_PX))
    assert worst <= LSTSQ_BAR_PX
